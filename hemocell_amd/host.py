"""Thin numpy-facing host layer over the C ABI.

Names follow the reference's interface for this path (hemocell.h:86-253,
core/hemoCellFields.h:103-158): latticeEquilibrium, collideAndStream,
spreadParticleForce, interpolateFluidVelocity, advanceParticles,
applyConstitutiveModel, iterate, setMaterialTimeScaleSeparation ...  Every
method is one call into libhemocell_amd.so; nothing is computed here.
"""
import ctypes as C
import math
import os
import xml.etree.ElementTree as ET

import numpy as np

from . import capi
from .capi import CellTypeSpec, HcError, Material, Params, WbcMaterial, check, dptr, lptr

HALO = 2

MODEL_RBC_HO = 0
MODEL_PLT_SIMPLE = 1
MODEL_WBC_HO = 2
MODEL_RBC_MALARIA = 3
IBM_PHI2, IBM_PHI3, IBM_PHI4 = 2, 3, 4   # hcp_type_set_ibm_kernel: nodes per axis of a type's IBM delta function
WBC_SPHERE = 0             # config/constant_defaults.h:83
RBC_FROM_SPHERE = 1        # config/constant_defaults.h:80
MESH_FROM_STL = 2          # config/constant_defaults.h:84
ELLIPSOID_FROM_SPHERE = 6  # config/constant_defaults.h:81

# examples/cell_shapes/WBC_HO.xml, kept as a data file with the test fixtures
WBC_HO_XML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "wbc_case",
                          "WBC_HO.xml")
# cases/stretchMalaria/RBC_MALARIA.xml; its <StlFile> is resolved next to it
MALARIA_XML = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "malaria_case",
                           "RBC_MALARIA.xml")

# examples/pipeflow/PLT.xml:14-38
PLT_INNER_EDGES = np.array([[60, 65], [62, 64], [37, 42], [54, 56], [34, 40], [25, 46], [50, 59], [29, 47],
                            [61, 63], [26, 45], [33, 43], [27, 35], [32, 39], [49, 51], [0, 4], [48, 52],
                            [6, 10], [53, 55], [19, 21], [57, 58], [15, 13]], dtype=np.int64)

_initialised = False


def _iptr(array):
    """a C int pointer to a contiguous numpy int32 array"""
    return array.ctypes.data_as(C.POINTER(C.c_int))


def read_material(path):
    """<MaterialModel> of a cell XML: {tag: float} for the numeric tags and "inner_edges" as an [n][2] int64 array
    (mechanics/commonCellConstants.cpp:139-153 reads <InnerEdges><Edge> a b </Edge>...)"""
    mm = ET.parse(path).getroot().find("MaterialModel")
    if mm is None:
        raise HcError("%s has no <MaterialModel>" % path)
    out = {}
    for el in mm:
        if el.tag == "InnerEdges":
            out["inner_edges"] = np.array([[int(v) for v in e.text.split()] for e in el.iter("Edge")], np.int64).reshape(-1, 2)
            continue
        try:
            out[el.tag] = float(el.text)
        except (TypeError, ValueError):
            pass
    return out


def read_stl_file_tag(path):
    """<MaterialModel><StlFile> of a cell XML, or None"""
    el = ET.parse(path).getroot().find("MaterialModel/StlFile")
    return None if el is None or not (el.text or "").strip() else el.text.strip()


def init(device=0):
    """plb::plbInit equivalent: select the GPU; raises if no gfx950 device."""
    global _initialised
    check(capi.lib().hc_init(device))
    _initialised = True


def ensure_init():
    if not _initialised:
        init(0)


def base_parameters(dx=5e-7, dt=1e-7, nuP=1.1e-6, rhoP=1025.0, kBT=4.100531391e-21):
    """param::lbm_base_parameters(cfg) (mechanics/constantConversion.cpp:36-59)"""
    P = Params()
    check(capi.lib().hc_params_base(C.byref(P), dx, dt, nuP, rhoP, kBT))
    return P


class Lattice:
    """One x-slab of the MultiBlockLattice3D<T,DESCRIPTOR> with GuoExternalForceBGKdynamics."""

    def __init__(self, nx, ny, nz, periodic=(False, False, False), omega=1.0, x0=0, nx_global=None, n_slabs=1):
        ensure_init()
        self.lib = capi.lib()
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.x0 = int(x0)
        self.nx_global = int(nx_global if nx_global is not None else nx)
        self.n_slabs = int(n_slabs)
        self.periodic = tuple(bool(p) for p in periodic)
        per = (C.c_int * 3)(*[int(p) for p in periodic])
        self.ptr = C.c_void_p()
        check(self.lib.hcl_create(C.byref(self.ptr), self.nx, self.ny, self.nz, per, float(omega),
                                  self.x0, self.nx_global, self.n_slabs))
        self.n = self.nx * self.ny * self.nz

    # defineDynamics(lattice, flagMatrix, bbox, new BounceBack(1.), 0)
    def defineBounceBack(self, mask_global):
        """mask_global: uint8 [nx_global][ny][nz] (1 = BounceBack).  The slab's halo planes are filled
        from the global array (periodic wrap in x if enabled, otherwise wall)."""
        m = np.ascontiguousarray(mask_global, dtype=np.uint8)
        if m.shape != (self.nx_global, self.ny, self.nz):
            raise HcError("mask must have the global shape %s, got %s" % ((self.nx_global, self.ny, self.nz), m.shape))
        xs = np.arange(self.x0 - HALO, self.x0 + self.nx + HALO)
        if self.periodic[0]:
            local = m[np.mod(xs, self.nx_global)]
        else:
            local = np.ones((len(xs), self.ny, self.nz), np.uint8)   # outside a non-periodic pipe end: wall
            ok = (xs >= 0) & (xs < self.nx_global)
            local[ok] = m[xs[ok]]
        local = np.ascontiguousarray(local)
        check(self.lib.hcl_set_mask(self.ptr, local.ctypes.data))

    def latticeEquilibrium(self, rho=1.0, u=(0.0, 0.0, 0.0)):
        uu = np.array(u, dtype=np.float64)
        check(self.lib.hcl_init_equilibrium(self.ptr, float(rho), dptr(uu)))

    def setExternalVector(self, F):
        ff = np.array(F, dtype=np.float64)
        check(self.lib.hcl_set_body_force(self.ptr, dptr(ff)))

    def setExternalVectorBoxes(self, boxes, forces):
        """setExternalVector on sub-domains (cases/kolmogorovFlow/kolmogorovFlow.cpp:136-140): inclusive global node boxes
        (x0, x1, y0, y1, z0, z1), later ones override earlier ones; an empty list removes them"""
        bb = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 6)
        ff = np.ascontiguousarray(forces, dtype=np.float64).reshape(-1, 3)
        assert len(bb) == len(ff)
        check(self.lib.hcl_set_body_force_regions(self.ptr, len(bb), _iptr(bb), dptr(ff)))

    def setBoundaryVelocity(self, wall_class, u):
        """wall_class an int: velocity of the nodes whose mask value is wall_class (3..6).  Otherwise wall_class is an
        inclusive box (x0, x1, y0, y1, z0, z1) or an [n][3] node list, and u one velocity or one per node ([n][3]) for its
        Zou-He velocity nodes (setBoundaryVelocity on nodes of addVelocityBoundary*)"""
        if isinstance(wall_class, (int, np.integer)):
            uu = np.array(u, dtype=np.float64)
            check(self.lib.hcl_set_wall_velocity(self.ptr, int(wall_class), dptr(uu)))
            return
        self._set_open(wall_class, u, 3, self.lib.hcl_open_boundary_set_velocity)

    def setBoundaryDensity(self, where, rho):
        """density of the Zou-He pressure nodes of a box or an [n][3] node list: one value or one per node"""
        self._set_open(where, rho, 1, self.lib.hcl_open_boundary_set_density)

    # Zou-He open boundaries (hcl_open_boundary_*), first with normal x.  Boxes are inclusive (x0, x1, y0, y1, z0, z1) in local
    # node coordinates; each call returns (first_slot, n): the nodes hold the slots first_slot .. first_slot + n - 1 in
    # box order (x outermost, z innermost)
    def addVelocityBoundary0N(self, box):
        return self._add_open_box(0, -1, box)

    def addVelocityBoundary0P(self, box):
        return self._add_open_box(0, 1, box)

    def addPressureBoundary0N(self, box):
        return self._add_open_box(1, -1, box)

    def addPressureBoundary0P(self, box):
        return self._add_open_box(1, 1, box)

    # ... and with normal y (1N / 1P) and z (2N / 2P): the same completion with the roles of x and the axis exchanged
    def addVelocityBoundary1N(self, box):
        return self._add_open_box(0, -1, box, 1)

    def addVelocityBoundary1P(self, box):
        return self._add_open_box(0, 1, box, 1)

    def addPressureBoundary1N(self, box):
        return self._add_open_box(1, -1, box, 1)

    def addPressureBoundary1P(self, box):
        return self._add_open_box(1, 1, box, 1)

    def addVelocityBoundary2N(self, box):
        return self._add_open_box(0, -1, box, 2)

    def addVelocityBoundary2P(self, box):
        return self._add_open_box(0, 1, box, 2)

    def addPressureBoundary2N(self, box):
        return self._add_open_box(1, -1, box, 2)

    def addPressureBoundary2P(self, box):
        return self._add_open_box(1, 1, box, 2)

    def addOpenBoundaryNodes(self, kind, orientation, nodes, axis=0):
        """kind 0 = velocity, 1 = pressure; orientation -1 = N, +1 = P; nodes [n][3]; axis 0, 1, 2: returns the first slot"""
        nn = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 3)
        first = C.c_int()
        check(self.lib.hcl_open_boundary_add_axis(self.ptr, int(kind), int(axis), int(orientation),
                                                  _iptr(nn), len(nn), C.byref(first)))
        return first.value

    def openBoundaryAxes(self, nodes):
        """the axis (0, 1, 2) on which each node of [n][3] was declared, or -1"""
        nn = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 3)
        out = np.empty(len(nn), np.int32)
        check(self.lib.hcl_open_boundary_axes(self.ptr, _iptr(nn), len(nn), _iptr(out)))
        return out

    def clearOpenBoundaries(self):
        check(self.lib.hcl_open_boundary_clear(self.ptr))

    def openBoundarySlots(self, nodes):
        nn = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1, 3)
        out = np.empty(len(nn), np.int32)
        check(self.lib.hcl_open_boundary_slots(self.ptr, _iptr(nn), len(nn), _iptr(out)))
        return out

    def setOpenBoundaryVelocitySlots(self, first_slot, u):
        uu = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 3)
        check(self.lib.hcl_open_boundary_set_velocity(self.ptr, int(first_slot), len(uu), uu.ctypes.data, 0))

    def setOpenBoundaryDensitySlots(self, first_slot, rho):
        rr = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        check(self.lib.hcl_open_boundary_set_density(self.ptr, int(first_slot), len(rr), rr.ctypes.data, 0))

    def openBoundaryValues(self, first_slot, n):
        """[n][4] (u_x, u_y, u_z, rho) of the slots"""
        out = np.empty((int(n), 4))
        check(self.lib.hcl_open_boundary_values(self.ptr, int(first_slot), int(n), dptr(out)))
        return out

    def planeVelocity(self, x, yz):
        """Cell::computeVelocity (u = j/rho + F/2, F the body force) on in-plane indices y * nz + z of plane x: [n][3]"""
        ii = np.ascontiguousarray(yz, dtype=np.int32).reshape(-1)
        out = np.empty((len(ii), 3))
        check(self.lib.hcl_plane_velocity(self.ptr, int(x), _iptr(ii), len(ii), out.ctypes.data, 0))
        return out

    def planeVelocityAxis(self, axis, plane, idx):
        """the same on the plane coordinate[axis] == plane: idx are in-plane indices as plane_index() forms them
        (y * nz + z, x * nz + z, x * ny + y for axis 0, 1, 2): [n][3]"""
        ii = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        out = np.empty((len(ii), 3))
        check(self.lib.hcl_plane_velocity_axis(self.ptr, int(axis), int(plane), _iptr(ii), len(ii),
                                               out.ctypes.data, 0))
        return out

    def _add_open_box(self, kind, orientation, box, axis=0):
        bb = (C.c_int * 6)(*[int(v) for v in box])
        first, n = C.c_int(), C.c_int()
        check(self.lib.hcl_open_boundary_add_box_axis(self.ptr, int(kind), int(axis), int(orientation), bb, C.byref(first), C.byref(n)))
        return first.value, n.value

    def _set_open(self, where, values, nc, fn):
        w = np.asarray(where)
        if w.shape == (6,):
            x0, x1, y0, y1, z0, z1 = [int(v) for v in w]
            g = np.mgrid[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1].reshape(3, -1).T
        else:
            g = w.reshape(-1, 3)
        slots = self.openBoundarySlots(g)
        if (slots < 0).any():
            raise HcError("node %s is not an open-boundary node" % (tuple(g[np.argmax(slots < 0)]),))
        v = np.asarray(values, dtype=np.float64)
        v = np.broadcast_to(v.reshape(-1, nc) if v.size != nc else v.reshape(1, nc), (len(g), nc))
        order = np.argsort(slots, kind="stable")
        s, vv = slots[order], np.ascontiguousarray(v[order])
        cut = np.flatnonzero(np.diff(s) != 1) + 1   # one call per run of consecutive slots
        for a, b in zip(np.r_[0, cut], np.r_[cut, len(s)]):
            blk = np.ascontiguousarray(vv[a:b])
            check(fn(self.ptr, int(s[a]), int(b - a), blk.ctypes.data, 0))

    def collideAndStream(self, steps=1):
        check(self.lib.hcl_collide_stream(self.ptr, int(steps)))

    # helper/leesEdwardsBC.h: the pass after every stream (hcl_set_lees_edwards)
    def setLeesEdwards(self, v_top, v_bottom):
        check(self.lib.hcl_set_lees_edwards(self.ptr, float(v_top), float(v_bottom)))

    def setLeesEdwardsDisplacement(self, D, d_per_iteration=0.0):
        """D for the next pass; d_per_iteration != 0: hc_iterate sets D = fmod(d * iter, nx) after every step"""
        check(self.lib.hcl_set_lees_edwards_displacement(self.ptr, float(D), float(d_per_iteration)))

    def applyLeesEdwards(self):
        """one pass on the current state (what Palabos' lattice->initialize() runs)"""
        check(self.lib.hcl_lees_edwards_apply(self.ptr))

    def leesEdwardsState(self):
        """(D, v_top, v_bottom, d_per_iteration)"""
        o = np.zeros(4)
        check(self.lib.hcl_lees_edwards_state(self.ptr, dptr(o)))
        return tuple(float(v) for v in o)

    def collide_part(self, part):
        check(self.lib.hcl_collide_stream_part(self.ptr, int(part)))

    def fluid_stats(self, what=0):
        """FluidInfo::calculate{Velocity,Force}Statistics: (min, max, mean, n) of |u| (what 0) or |F| (what 1) over
        the non-boundary nodes, reduced on the device"""
        o = np.zeros(3); n = C.c_long()
        check(self.lib.hcl_fluid_stats(self.ptr, int(what), dptr(o), C.byref(n)))
        return o[0], o[1], (o[2] / n.value if n.value else 0.0), n.value

    def step_end(self):
        check(self.lib.hcl_step_end(self.ptr))

    def populations(self):
        """[n][19] post-stream populations (f - t_i), reference node order z + nz*(y + ny*x)"""
        out = np.empty((self.n, 19), dtype=np.float64)
        check(self.lib.hcl_download_populations(self.ptr, dptr(out)))
        return out

    def set_populations(self, f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.shape != (self.n, 19):
            raise HcError("populations must have shape (%d, 19), got %s" % (self.n, f.shape))
        check(self.lib.hcl_upload_populations(self.ptr, dptr(f)))

    def rho_u(self):
        rho = np.empty(self.n, dtype=np.float64)
        u = np.empty((self.n, 3), dtype=np.float64)
        check(self.lib.hcl_download_rho_u(self.ptr, dptr(rho), dptr(u)))
        return rho, u

    def pi_neq(self):
        """off-equilibrium momentum flux (xx, xy, xz, yy, yz, zz) per node"""
        pi = np.empty((self.n, 6), dtype=np.float64)
        check(self.lib.hcl_download_pi_neq(self.ptr, dptr(pi)))
        return pi

    def ibm_force(self):
        F = np.empty((self.n, 3), dtype=np.float64)
        check(self.lib.hcl_download_ibm_force(self.ptr, dptr(F)))
        return F

    def halo_doubles(self, width):
        return int(self.lib.hcl_halo_doubles(self.ptr, int(width)))

    def halo_pack(self, side, width, dev_ptr, next=False):
        fn = self.lib.hcl_halo_pack_next if next else self.lib.hcl_halo_pack
        check(fn(self.ptr, int(side), int(width), C.c_void_p(dev_ptr)))

    def halo_unpack(self, side, width, dev_ptr):
        check(self.lib.hcl_halo_unpack(self.ptr, int(side), int(width), C.c_void_p(dev_ptr)))

    def bytes_per_node(self):
        return float(self.lib.hcl_mlups_bytes_per_node(self.ptr))

    # interior viscosity (INTERIOR_VISCOSITY builds of the reference): a class byte per node picks the omega a fluid node
    # relaxes with -- 0 the lattice's, k >= 1 omegas[k - 1]
    def enableInteriorViscosity(self, omegas):
        oo = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        check(self.lib.hcl_interior_enable(self.ptr, len(oo), dptr(oo)))

    def interiorViscosityOmegas(self):
        """the omegas of the classes 1 .. n; empty while the feature is off"""
        n = C.c_int()
        oo = np.zeros(7)
        check(self.lib.hcl_interior_info(self.ptr, C.byref(n), dptr(oo)))
        return oo[:n.value].copy()

    def setInteriorClasses(self, classes):
        cc = np.ascontiguousarray(classes, dtype=np.uint8)
        if cc.size != self.n:
            raise HcError("classes must have %d entries, got %d" % (self.n, cc.size))
        check(self.lib.hcl_interior_upload_classes(self.ptr, cc.ctypes.data))

    def interiorClasses(self):
        """uint8 [nx][ny][nz]: the class of every node"""
        out = np.empty((self.nx, self.ny, self.nz), dtype=np.uint8)
        check(self.lib.hcl_interior_download_classes(self.ptr, out.ctypes.data))
        return out

    # solidify mechanics (SOLIDIFY_MECHANICS builds of the reference): the binding field, one byte per node
    def populateBindingSites(self, box):
        """populateBindingSites(box): every boundary node of the inclusive box (x0, x1, y0, y1, z0, z1) with a fluid node
        among its 26 neighbours becomes a binding site; calls add up"""
        b = [int(v) for v in box]
        if len(b) != 6:
            raise HcError("a box is (x0, x1, y0, y1, z0, z1), got %r" % (box,))
        check(self.lib.hcl_binding_populate(self.ptr, (C.c_int * 6)(*b)))

    def bindingSites(self):
        """uint8 [nx][ny][nz]: 1 = a binding site"""
        out = np.empty((self.nx, self.ny, self.nz), dtype=np.uint8)
        check(self.lib.hcl_binding_download(self.ptr, out.ctypes.data))
        return out

    def setBindingSites(self, sites):
        ss = np.ascontiguousarray(sites, dtype=np.uint8)
        if ss.size != self.n:
            raise HcError("the binding field must have %d entries, got %d" % (self.n, ss.size))
        check(self.lib.hcl_binding_upload(self.ptr, ss.ctypes.data))

    def clearBindingSites(self):
        check(self.lib.hcl_binding_clear(self.ptr))

    def mask(self):
        """uint8 [nx][ny][nz]: the mask classes the device holds now (0 fluid, 1 bounce-back, 2 inert solid, 3..6 moving
        walls), nodes solidified since defineBounceBack included"""
        out = np.empty((self.nx, self.ny, self.nz), dtype=np.uint8)
        check(self.lib.hcl_download_mask(self.ptr, out.ctypes.data))
        return out

    def node_counts(self):
        """(nodes, fluid nodes, nodes the collide visits)"""
        o = (C.c_long * 3)()
        check(self.lib.hcl_node_counts(self.ptr, o))
        return tuple(int(v) for v in o)

    def tresca(self):
        """eigenValueFromCell per node: (lambda_max - lambda_min) / 2 of S = -omega 3 / (2 rho) PiNeq; 0 off the fluid"""
        out = np.empty(self.n, dtype=np.float64)
        check(self.lib.hcl_download_tresca(self.ptr, dptr(out)))
        return out

    def createCEPACfield(self, tau):
        """the CEPAC scalar field of this lattice (core/hemoCellFields.cpp:120-133), relaxing with omega = 1 / tau:
        diffusivity (tau - 0.5) / 3 in lattice units"""
        if not tau > 0.0:
            raise HcError("createCEPACfield: tau must be positive, got %r" % (tau,))
        self.scalar = Scalar(self, 1.0 / float(tau))
        return self.scalar

    def destroy(self):
        if self.ptr:
            check(self.lib.hcl_destroy(self.ptr))   # takes the lattice's scalar field with it
            if getattr(self, "scalar", None) is not None:
                self.scalar.ptr = C.c_void_p()
            self.ptr = C.c_void_p()


class Scalar:
    """The CEPAC field: a passive scalar (a dissolved agonist concentration C) that the lattice's flow carries and that
    diffuses.  Arrays are in the lattice's node order z + nz*(y + ny*x)."""

    def __init__(self, lattice, omega):
        self.lib = capi.lib()
        self.lattice = lattice
        self.omega = float(omega)
        self.ptr = C.c_void_p()
        check(self.lib.hcl_scalar_create(lattice.ptr, self.omega, C.byref(self.ptr)))
        self.n = lattice.n

    @staticmethod
    def _box(box):
        b = [int(v) for v in box]
        if len(b) != 6:
            raise HcError("a box is (x0, x1, y0, y1, z0, z1), got %r" % (box,))
        return (C.c_int * 6)(*b)

    def initializeAtEquilibrium(self, C_value, box=None):
        """plb::initializeAtEquilibrium(field, box, C, u) at u = 0; box: inclusive node ranges, None = every node"""
        check(self.lib.hcl_scalar_init_equilibrium(self.ptr, self._box(box) if box is not None else None, float(C_value)))

    def addSource(self, box, C_value):
        """the nodes of the box hold C from now on (setBoundaryDensity on the temperature boundary of the reference's case)"""
        check(self.lib.hcl_scalar_set_source_box(self.ptr, self._box(box), float(C_value)))

    def clearSources(self):
        check(self.lib.hcl_scalar_clear_sources(self.ptr))

    def collideAndStream(self):
        """one step with the velocity of the lattice's present state (after Lattice.step_end or collideAndStream)"""
        check(self.lib.hcl_scalar_step(self.ptr))

    def concentration(self):
        out = np.empty(self.n, dtype=np.float64)
        check(self.lib.hcl_scalar_download(self.ptr, dptr(out)))
        return out

    def velocity(self):
        """[n][3]: the velocity the next step advects with; 0 on nodes that are not fluid"""
        out = np.empty((self.n, 3), dtype=np.float64)
        check(self.lib.hcl_scalar_download_velocity(self.ptr, dptr(out)))
        return out

    def populations(self):
        """[n][19] post-stream populations (g - t_i)"""
        out = np.empty((self.n, 19), dtype=np.float64)
        check(self.lib.hcl_scalar_download_populations(self.ptr, dptr(out)))
        return out

    def set_populations(self, g):
        g = np.ascontiguousarray(g, dtype=np.float64)
        if g.shape != (self.n, 19):
            raise HcError("populations must have shape (%d, 19), got %s" % (self.n, g.shape))
        check(self.lib.hcl_scalar_upload_populations(self.ptr, dptr(g)))

    def stats(self):
        """(sum, minimum, maximum) of C over the fluid nodes, reduced on the device"""
        o = np.zeros(3)
        check(self.lib.hcl_scalar_stats(self.ptr, dptr(o)))
        return o[0], o[1], o[2]

    def destroy(self):
        if self.ptr:
            check(self.lib.hcl_scalar_destroy(self.ptr))
            self.ptr = C.c_void_p()
            if getattr(self.lattice, "scalar", None) is self:
                self.lattice.scalar = None


class LeesEdwardsBC:
    """hemo::LeesEdwardsBC (helper/leesEdwardsBC.h): shear along x between the z faces of an all-periodic lattice.
    shear_rate_lbm is param::shearrate_lbm; the displacement per iteration is shear_rate_lbm * dt, as the reference has it."""

    def __init__(self, lattice, shear_rate_lbm, dt):
        self.lattice = lattice
        self.nx, self.ny, self.nz = lattice.nx_global, lattice.ny, lattice.nz
        self.dt = dt
        self.LEdisplacement = shear_rate_lbm * dt
        v_half = (self.nz - 1) * shear_rate_lbm * 0.5
        self.topVelocity = -v_half
        self.bottomVelocity = v_half
        self.LEcurrentDisplacement = 0.0

    def initialize(self, schedule=True):
        """periodicity is the lattice's (all three axes); the pass starts with D = 0.  schedule: hc_iterate advances D as
        updateLECurDisplacement(iter) after every iteration would"""
        self.lattice.setLeesEdwards(self.topVelocity, self.bottomVelocity)
        self.lattice.setLeesEdwardsDisplacement(0.0, self.LEdisplacement if schedule else 0.0)

    def updateLECurDisplacement(self, it):
        self.LEcurrentDisplacement = math.fmod(self.LEdisplacement * it, float(self.nx))
        self.lattice.setLeesEdwardsDisplacement(self.LEcurrentDisplacement, self.lattice.leesEdwardsState()[3])


def preinlet_driving_force(Re, nu_lbm, fluid_area, direction="Xpos"):
    """PreInlet::calculateDrivingForce (helper/preInlet.cpp): the pipe radius R = sqrt(A / pi) of the gathered number A of
    fluid nodes of the pre-inlet's plane 2 in from its upstream end, u_max = Re nu / (2 R) and the driving force
    8 nu (u_max / 2) / R / R in the reference's operation order, along -x for Xpos and +x for Xneg.  Returns (R, u_max, F_x)."""
    if direction not in ("Xpos", "Xneg"):
        raise HcError("PreInlet: only the directions Xpos and Xneg are supported")
    radius, u_max, F = preinlet_driving_force_vector(Re, nu_lbm, fluid_area, direction)
    return radius, u_max, F[0]


# the reference's six Direction values (helper/preInlet.h): name -> (axis, -1 for *neg / +1 for *pos)
PREINLET_DIRECTIONS = {"Xneg": (0, -1), "Xpos": (0, 1), "Yneg": (1, -1), "Ypos": (1, 1), "Zneg": (2, -1), "Zpos": (2, 1)}


def _preinlet_direction(direction):
    if direction not in PREINLET_DIRECTIONS:
        raise HcError("PreInlet: unknown direction %r (Xneg, Xpos, Yneg, Ypos, Zneg, Zpos)" % (direction,))
    return PREINLET_DIRECTIONS[direction]


def preinlet_driving_force_vector(Re, nu_lbm, fluid_area, direction):
    """preinlet_driving_force in any of the six directions (PreInlet::calculateDrivingForce in the reference's operation
    order): the force on the direction's axis, + for *neg and - for *pos (setDrivingForce), zero
    on the other axes.  Returns (R, u_max, (F_x, F_y, F_z))."""
    axis, sign = _preinlet_direction(direction)
    radius = math.sqrt(fluid_area / math.pi)
    u_max = Re * nu_lbm / (radius * 2)
    force = 8 * nu_lbm * (u_max * 0.5) / radius / radius
    F = [0.0, 0.0, 0.0]
    F[axis] = -force if sign > 0 else force
    return radius, u_max, tuple(F)


def plane_index(dims, axis, a, b):
    """the in-plane index hcl_plane_velocity_axis takes: the node's offset with `axis` removed and the remaining axes in
    lattice order.  a, b: the coordinates on the two other axes in ascending axis order -- (y, z), (x, z), (x, y) for axis
    0, 1, 2 -- so the index is y * nz + z, x * nz + z, x * ny + y.  dims: (nx, ny, nz).  Pure numpy."""
    if axis not in (0, 1, 2):
        raise HcError("plane_index: axis must be 0, 1 or 2")
    inner = dims[1] if axis == 2 else dims[2]
    return np.asarray(a, dtype=np.int64) * int(inner) + np.asarray(b, dtype=np.int64)


class PreInlet:
    """One-process stand-in for helper/preInlet.h's fluid coupling in the reference's six directions: a pre-inlet lattice and a
    domain lattice step in the reference's per-iteration order -- both iterate, then applyPreInlet: the pre-inlet evaluates
    u = j/rho + F/2 on its plane pre_x at the coupled nodes, and the domain takes them as the velocities of its Zou-He velocity
    nodes at the same global in-plane coordinates on its plane domain_x.  The domain thus lags the pre-inlet by one iteration,
    as in the reference.  For a direction on axis a (X: 0, Y: 1, Z: 2), pre_x and domain_x are plane numbers along a, the
    domain's inlet is an <a>N side for *neg (the pre-inlet lies below the domain and drives along +a) and an <a>P side for
    *pos, and yz: [n][2] holds the GLOBAL coordinates of the coupled nodes on the two other axes in ascending axis order --
    (y, z), (x, z), (x, y); pre_origin / domain_origin likewise: the global in-plane coordinates of each lattice's node 0 of
    those axes -- the cross-sections may differ, as the reference's pre-inlet box (the slice's bounding box enlarged by 1)
    differs from the domain's.  device=False: applyPreInlet reads the plane velocities back and sets the slots from the host
    (two waits for the stream per iteration); it and iterate return the velocities sent.  device=True: an hc_preinlet handle
    (hcl_preinlet_*) does the exchange in one kernel, iterate(n) queues all n iterations in one call, and both return None;
    sent() reads the slots back either way.  A device coupling holds pointers into both lattices: destroy() it before them.
    Cells cross with cells=(pre_cells, domain_cells) (device=True only; helper/preInlet.cpp:254-351,
    applyPreInletParticleBoundary): a complete cell of the pre-inlet whose whole vertex set lies in window=(lo, hi) along the
    axis, positions taken modulo the pre-inlet's length lap by lap, is copied into the domain at p + shift with the id
    id + (lap - sign) * id_stride; sink=plane removes the domain's cells that reach past that plane downstream.  iterate(n) is
    then one hc_preinlet_iterate -- both systems step with their cells (particle_timescale, force_limit,
    deletion_check_every), the fluid is handed over, and every cells_every iterations the cells are checked (one host wait per
    check); applyPreInletCells() is one check, cell_counts() = (injected, rejected, removed by the sink, checks).  Partly
    arrived cells are never added.  Without cells= the coupling is the fluid's alone.
    The domain may be one x-slab of a multi-rank run (n_slabs > 1) for the fluid coupling along x: the object lives on the rank
    that holds the inlet plane -- rank 0 with plane 0 for Xneg, the last rank with plane nx - 1 for Xpos -- beside its own
    whole pre-inlet lattice; domain_x is that rank's local plane and the slots are its local slots.  The domain's step inside
    iterate(n) is then collective: every other rank steps its slab the same number of times (collideAndStream(n) or
    HemoCell.iterate(n)).  With cells=(pre_cells, slab_cells) the cells cross into the slabs too (hcp_preinlet_create_slab):
    constructing the object, iterate(n) and applyPreInletCells() are then collective, and every other rank holds a
    PreInletPeer made with the same window, shift, id_stride, sink and cadences and makes the same calls.  shift and sink are
    in GLOBAL domain coordinates; the window's image [lo + shift_x, hi + shift_x] must lie in the inlet rank's slab, at least the
    particle envelope away from its inner face, so that an arriving cell is held by the inlet rank alone until the envelope
    synchronisation replicates it.  The sink takes a cell from every rank that holds it in the same check, and cell_counts()
    are totals over the whole domain, equal on every rank.  With hc_set_reproducible_spread(1) the slabs hold the bits of the
    same run on one domain.  Other directions, a pre-inlet on slabs and partly arrived cells are refused."""

    def __init__(self, preinlet, domain, yz, pre_x, domain_x, direction="Xpos", pre_origin=(0, 0), domain_origin=(0, 0),
                 device=False, cells=None, window=None, shift=(0.0, 0.0, 0.0), id_stride=None, sink=None, cells_every=1,
                 particle_timescale=1, force_limit=True, deletion_check_every=1):
        axis, sign = _preinlet_direction(direction)
        if getattr(preinlet, "n_slabs", 1) != 1:
            raise HcError("PreInlet: the pre-inlet lattice needs n_slabs = 1 (it lives whole on the rank that holds the inlet plane)")
        if getattr(domain, "n_slabs", 1) != 1 and axis != 0:
            raise HcError("PreInlet: direction %s needs n_slabs = 1 on the domain; a slab is fed along x only "
                          "(Xneg on rank 0, Xpos on the last rank)" % direction)
        if cells is not None:
            if not device:
                raise HcError("PreInlet: cells= needs device=True (the cells cross on the device)")
            if window is None or id_stride is None:
                raise HcError("PreInlet: cells= needs window=(lo, hi) and id_stride=")
            if int(cells_every) < 1:
                raise HcError("PreInlet: cells_every must be >= 1")
        self.pre, self.domain = preinlet, domain   # kept alive as long as the coupling
        self.axis, self.device, self.ptr = axis, bool(device), None
        others = [d for d in range(3) if d != axis]
        pdims, ddims = (preinlet.nx, preinlet.ny, preinlet.nz), (domain.nx, domain.ny, domain.nz)
        g = np.asarray(yz, dtype=np.int64).reshape(-1, 2)
        pa, pb = g[:, 0] - int(pre_origin[0]), g[:, 1] - int(pre_origin[1])
        da, db = g[:, 0] - int(domain_origin[0]), g[:, 1] - int(domain_origin[1])
        if ((pa < 0) | (pa >= pdims[others[0]]) | (pb < 0) | (pb >= pdims[others[1]])).any():
            raise HcError("PreInlet: a coupled node lies outside the pre-inlet's cross-section")
        if ((da < 0) | (da >= ddims[others[0]]) | (db < 0) | (db >= ddims[others[1]])).any():
            raise HcError("PreInlet: a coupled node lies outside the domain's cross-section")
        self.pre_yz = np.ascontiguousarray(plane_index(pdims, axis, pa, pb), dtype=np.int32)
        self.pre_x, self.domain_x = int(pre_x), int(domain_x)
        nodes = np.empty((len(g), 3), np.int64)
        nodes[:, axis], nodes[:, others[0]], nodes[:, others[1]] = self.domain_x, da, db
        self.domain_nodes = nodes
        # *neg: the pre-inlet lies below the domain and drives along +axis, so the domain's inlet is an N side; *pos mirrors it
        # (initializePreInletVelocityBoundary: addVelocityBoundary<axis>N / <axis>P)
        self.first = domain.addOpenBoundaryNodes(0, sign, self.domain_nodes, axis=axis)
        if self.device:
            ptr = C.c_void_p()
            check(capi.lib().hcl_preinlet_create(C.byref(ptr), preinlet.ptr, domain.ptr, axis, self.pre_x,
                                                 _iptr(self.pre_yz), len(self.pre_yz), self.first))
            self.ptr = ptr
        if cells is not None:
            self.cells, self.cells_ptr, self.iter = tuple(cells), None, 0
            self.cells_every, self.particle_timescale = int(cells_every), int(particle_timescale)
            self.force_limit, self.deletion_check_every = bool(force_limit), int(deletion_check_every)
            sh = np.array(shift, dtype=np.float64).reshape(3)
            xp = C.c_void_p()
            # a slab of a multi-rank run: the collective entry point, which the other ranks reach through PreInletPeer
            create = capi.lib().hcp_preinlet_create if getattr(domain, "n_slabs", 1) == 1 else capi.lib().hcp_preinlet_create_slab
            try:
                check(create(C.byref(xp), self.cells[0].ptr, self.cells[1].ptr, axis, sign,
                             float(window[0]), float(window[1]), dptr(sh), int(id_stride)))
                self.cells_ptr = xp
                if sink is not None:
                    check(capi.lib().hcp_preinlet_set_sink(xp, 1, float(sink)))
            except HcError:
                self.destroy()
                raise

    def applyPreInletCells(self):
        """one check: the sink, then the injection; returns (cells injected, cells removed by the sink)"""
        a, b = C.c_long(), C.c_long()
        check(capi.lib().hcp_preinlet_apply(self._cells_handle(), C.byref(a), C.byref(b)))
        return a.value, b.value

    def cell_counts(self):
        """(cells injected, rejected, removed by the sink, checks) since the coupling was made"""
        out = np.zeros(4, dtype=np.int64)
        check(capi.lib().hcp_preinlet_counts(self._cells_handle(), lptr(out)))
        return tuple(int(v) for v in out)

    def _cells_handle(self):
        if getattr(self, "cells_ptr", None) is None:
            raise HcError("PreInlet: no cell coupling (cells= was not given, or it has been destroyed)")
        return self.cells_ptr

    def applyPreInlet(self):
        if self.device:
            check(capi.lib().hcl_preinlet_apply(self._handle()))
            return None
        u = self.pre.planeVelocityAxis(self.axis, self.pre_x, self.pre_yz)
        self.domain.setOpenBoundaryVelocitySlots(self.first, u)
        return u

    def iterate(self, n=1):
        """n iterations of (pre-inlet step, domain step, applyPreInlet).  Host path: returns the last plane velocities sent;
        device path: one hcl_preinlet_iterate, nothing waits for the device, returns None"""
        if getattr(self, "cells_ptr", None) is not None:
            it = C.c_long(self.iter)
            try:
                check(capi.lib().hc_preinlet_iterate(self._handle(), self.cells_ptr, C.byref(it), int(n), self.particle_timescale,
                                                     int(self.force_limit), self.deletion_check_every, self.cells_every))
            finally:
                self.iter = it.value
            return None
        if self.device:
            check(capi.lib().hcl_preinlet_iterate(self._handle(), int(n)))
            return None
        u = None
        for _ in range(int(n)):
            self.pre.collideAndStream(1)
            self.domain.collideAndStream(1)
            u = self.applyPreInlet()
        return u

    def sent(self):
        """[n][3]: the velocities the domain's coupled slots hold now"""
        return self.domain.openBoundaryValues(self.first, len(self.pre_yz))[:, :3]

    def _handle(self):
        if self.ptr is None:
            raise HcError("PreInlet: the device coupling has been destroyed")
        return self.ptr

    def destroy(self):
        """frees the device coupling, if any; call it before destroying either lattice or cell container"""
        if getattr(self, "cells_ptr", None) is not None:
            check(capi.lib().hcp_preinlet_destroy(self.cells_ptr))
            self.cells_ptr = None
        if self.ptr is not None:
            check(capi.lib().hcl_preinlet_destroy(self.ptr))
            self.ptr = None


class PreInletPeer:
    """What a rank WITHOUT the inlet plane holds while the inlet rank holds PreInlet(..., cells=(pre_cells, slab_cells)) over a
    domain cut into x-slabs: the same collective handle (hcp_preinlet_create_slab with no pre-inlet), made with the same
    direction, window, shift, id_stride, sink and cadences, and the same calls -- iterate(n) steps this rank's slab and joins
    the check every cells_every iterations, applyPreInletCells() is one check, cell_counts() the global totals.  Every rank
    constructs its object, calls and destroys it in the same order as the inlet rank does."""

    def __init__(self, domain_cells, direction="Xneg", window=None, shift=(0.0, 0.0, 0.0), id_stride=None, sink=None,
                 cells_every=1, particle_timescale=1, force_limit=True, deletion_check_every=1):
        axis, sign = _preinlet_direction(direction)
        if window is None or id_stride is None:
            raise HcError("PreInletPeer: needs window=(lo, hi) and id_stride=, as the inlet rank's PreInlet")
        if int(cells_every) < 1:
            raise HcError("PreInletPeer: cells_every must be >= 1")
        self.cells, self.cells_ptr, self.iter = (None, domain_cells), None, 0
        self.cells_every, self.particle_timescale = int(cells_every), int(particle_timescale)
        self.force_limit, self.deletion_check_every = bool(force_limit), int(deletion_check_every)
        sh = np.array(shift, dtype=np.float64).reshape(3)
        xp = C.c_void_p()
        check(capi.lib().hcp_preinlet_create_slab(C.byref(xp), None, domain_cells.ptr, axis, sign, float(window[0]),
                                                  float(window[1]), dptr(sh), int(id_stride)))
        self.cells_ptr = xp
        if sink is not None:
            check(capi.lib().hcp_preinlet_set_sink(xp, 1, float(sink)))

    applyPreInletCells = PreInlet.applyPreInletCells
    cell_counts = PreInlet.cell_counts
    _cells_handle = PreInlet._cells_handle

    def iterate(self, n=1):
        it = C.c_long(self.iter)
        try:
            check(capi.lib().hc_preinlet_iterate(None, self._cells_handle(), C.byref(it), int(n), self.particle_timescale,
                                                 int(self.force_limit), self.deletion_check_every, self.cells_every))
        finally:
            self.iter = it.value

    def destroy(self):
        if self.cells_ptr is not None:
            check(capi.lib().hcp_preinlet_destroy(self.cells_ptr))
            self.cells_ptr = None


class CellType:
    """hemocell.addCellType<Mechanics>(name, constructType) for one type."""

    def __init__(self, P, model, shape, radius, min_triangles, kLink, kArea, kVolume, kBend, eta_m=0.0,
                 aspect_ratio=0.3, inner_edges=None, wbc=None, kInnerLink=None, stl=None, ex=False,
                 interior_viscosity=False, viscosity_ratio=None, solidify=None):
        """solidify: (distanceThreshold in lattice units, shearThreshold) of the cell XML's <MaterialModel>, for
        MODEL_PLT_SIMPLE: Cells.addCellType then enables solidify mechanics for the type (enableSolidifyMechanics).
        interior_viscosity, viscosity_ratio: <enableInteriorViscosity> and <viscosityRatio> of the cell XML
        (core/hemoCellField.cpp:100-112): Cells.addCellType then marks the type with tau_int = ratio (tau - 0.5) + 0.5.
        wbc: (kInnerRigid, kCytoskeleton, coreRadius, radius) in SI units, for MODEL_WBC_HO only;
        kInnerLink: for MODEL_RBC_MALARIA only; stl: the STL file of shape MESH_FROM_STL (any model).
        The malaria model, STL meshes and ex=True go through hcp_celltype_create_ex, the rest through the entry point
        of their model"""
        ensure_init()
        self.lib = capi.lib()
        M = Material()
        M.kLink, M.kArea, M.kVolume, M.kBend, M.eta_m = kLink, kArea, kVolume, kBend, eta_m
        M.radius, M.min_triangles, M.aspect_ratio = radius, int(min_triangles), aspect_ratio
        self._ie = None
        if inner_edges is not None and len(inner_edges):
            self._ie = np.ascontiguousarray(inner_edges, dtype=np.int64)
            M.inner_edges = lptr(self._ie)
            M.n_inner = len(self._ie)
        else:
            M.inner_edges = None
            M.n_inner = 0
        self.ptr = C.c_void_p()
        if (stl is not None) != (shape == MESH_FROM_STL):
            raise HcError("an STL file goes with shape MESH_FROM_STL, and that shape needs one")
        if (kInnerLink is not None) != (model == MODEL_RBC_MALARIA):
            raise HcError("kInnerLink goes with MODEL_RBC_MALARIA, and that model needs it")
        W = None
        if model == MODEL_WBC_HO:
            if wbc is None:
                raise HcError("MODEL_WBC_HO needs wbc=(kInnerRigid, kCytoskeleton, coreRadius, radius)")
            W = WbcMaterial(*[float(v) for v in wbc])
        if ex or model == MODEL_RBC_MALARIA or shape == MESH_FROM_STL:
            S = CellTypeSpec(model=int(model), shape=int(shape), material=M, kInnerLink=float(kInnerLink or 0.0),
                             stl_path=None if stl is None else os.fsencode(stl))
            S.wbc = C.pointer(W) if W is not None else None
            self._spec = (S, W)
            check(self.lib.hcp_celltype_create_ex(C.byref(self.ptr), C.byref(P), C.byref(S)))
        elif model == MODEL_WBC_HO:
            if wbc is None:
                raise HcError("MODEL_WBC_HO needs wbc=(kInnerRigid, kCytoskeleton, coreRadius, radius)")
            W = WbcMaterial(*[float(v) for v in wbc])
            check(self.lib.hcp_celltype_create_wbc(C.byref(self.ptr), int(shape), C.byref(P), C.byref(M), C.byref(W)))
        else:
            check(self.lib.hcp_celltype_create(C.byref(self.ptr), int(model), int(shape), C.byref(P), C.byref(M)))
        sz = (C.c_int * 4)()
        check(self.lib.hcp_celltype_sizes(self.ptr, sz))
        self.nv, self.nt, self.ne, self.nie = [int(x) for x in sz]
        self.model = model
        if interior_viscosity and viscosity_ratio is None:
            raise HcError("interior_viscosity=True needs viscosity_ratio=")
        self.interior_viscosity = bool(interior_viscosity)
        self.solidify = None if solidify is None else (float(solidify[0]), float(solidify[1]))
        self.interiorViscosityTau = None if viscosity_ratio is None else float(viscosity_ratio) * (P.tau - 0.5) + 0.5

    @classmethod
    def rbc(cls, P, **kw):
        """examples/pipeflow/RBC.xml with RbcHighOrderModel / RBC_FROM_SPHERE (MESH_FROM_STL when stl= is given)"""
        d = dict(radius=3.91e-6, min_triangles=600, kLink=15.0, kArea=5.0, kVolume=20.0, kBend=80.0, eta_m=0.0)
        d.update(kw)
        return cls(P, MODEL_RBC_HO, MESH_FROM_STL if d.get("stl") is not None else RBC_FROM_SPHERE, **d)

    @classmethod
    def plt(cls, P, **kw):
        """examples/pipeflow/PLT.xml with PltSimpleModel / ELLIPSOID_FROM_SPHERE (MESH_FROM_STL when stl= is given)"""
        d = dict(radius=1.25e-6, min_triangles=66, kLink=25.0, kArea=8.0, kVolume=100.0, kBend=250.0, eta_m=0.0,
                 aspect_ratio=0.434782608696, inner_edges=PLT_INNER_EDGES)
        d.update(kw)
        return cls(P, MODEL_PLT_SIMPLE, MESH_FROM_STL if d.get("stl") is not None else ELLIPSOID_FROM_SPHERE, **d)

    @classmethod
    def malaria(cls, P, xml=None, stl=None, **kw):
        """RbcMalariaModel on MESH_FROM_STL with the moduli, kInnerLink and inner edges of a malaria XML (default:
        cases/stretchMalaria/RBC_MALARIA.xml) and the STL file its <StlFile> names, found next to the XML unless stl= is
        given; keyword arguments override single values, kInnerLink included"""
        xml = xml or MALARIA_XML
        m = read_material(xml)
        if stl is None:
            tag = read_stl_file_tag(xml)
            if tag is None:
                raise HcError("%s has no <StlFile>" % xml)
            stl = os.path.join(os.path.dirname(os.path.abspath(xml)), tag)
        d = dict(radius=m["radius"], min_triangles=int(m.get("minNumTriangles", 0)), kLink=m["kLink"], kArea=m["kArea"],
                 kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"], inner_edges=m.get("inner_edges"),
                 kInnerLink=m["kInnerLink"])
        d.update(kw)
        return cls(P, MODEL_RBC_MALARIA, MESH_FROM_STL, stl=stl, **d)

    def malaria_constants(self):
        """lattice-unit k_inner_link of an RBC_MALARIA type (0 for the other models)"""
        out = np.zeros(1)
        check(self.lib.hcp_celltype_malaria_constants(self.ptr, dptr(out)))
        return dict(k_inner_link=float(out[0]))

    @classmethod
    def wbc(cls, P, xml=None, shape=WBC_SPHERE, **kw):
        """WbcHighOrderModel on WBC_SPHERE with the moduli, WBC constants and inner edges of a WBC XML
        (default: examples/cell_shapes/WBC_HO.xml); keyword arguments override single values, including
        kInnerRigid, kCytoskeleton, coreRadius and wbc_radius (the cytoskeleton radius, default the mesh radius)"""
        m = read_material(xml or WBC_HO_XML)
        d = dict(radius=m["radius"], min_triangles=int(m["minNumTriangles"]), kLink=m["kLink"], kArea=m["kArea"],
                 kVolume=m["kVolume"], kBend=m["kBend"], eta_m=m["eta_m"], aspect_ratio=m.get("aspectRatio", 0.3),
                 inner_edges=m.get("inner_edges"))
        w = dict(kInnerRigid=m["kInnerRigid"], kCytoskeleton=m["kCytoskeleton"], coreRadius=m["coreRadius"],
                 wbc_radius=m["radius"])
        for k in list(kw):
            if k in w:
                w[k] = kw.pop(k)
        d.update(kw)
        return cls(P, MODEL_WBC_HO, shape, wbc=(w["kInnerRigid"], w["kCytoskeleton"], w["coreRadius"], w["wbc_radius"]), **d)

    def wbc_constants(self):
        """lattice-unit (k_inner_rigid, k_cytoskeleton, core_radius, radius) of a WBC_HO type"""
        out = np.zeros(4)
        check(self.lib.hcp_celltype_wbc_constants(self.ptr, dptr(out)))
        return dict(zip(("k_inner_rigid", "k_cytoskeleton", "core_radius", "radius"), out.tolist()))

    def tables(self):
        t = dict(vertices=np.empty((self.nv, 3)), triangles=np.empty((self.nt, 3), np.int64),
                 edges=np.empty((self.ne, 2), np.int64), edge_length_eq=np.empty(self.ne),
                 edge_angle_eq=np.empty(self.ne), triangle_area_eq=np.empty(self.nt),
                 vertex_vertexes=np.empty((self.nv, 6), np.int64), patch_dist_eq=np.empty(self.nv),
                 scalars=np.empty(9))
        check(self.lib.hcp_celltype_tables(self.ptr, dptr(t["vertices"]), lptr(t["triangles"]), lptr(t["edges"]),
                                           dptr(t["edge_length_eq"]), dptr(t["edge_angle_eq"]),
                                           dptr(t["triangle_area_eq"]), lptr(t["vertex_vertexes"]),
                                           dptr(t["patch_dist_eq"]), dptr(t["scalars"])))
        names = ("volume_eq", "area_mean_eq", "edge_mean_eq", "angle_mean_eq", "k_volume", "k_area", "k_link",
                 "k_bend", "eta_m")
        t.update({n: float(v) for n, v in zip(names, t["scalars"])})
        return t

    def destroy(self):
        if self.ptr:
            check(self.lib.hcp_celltype_destroy(self.ptr))
            self.ptr = C.c_void_p()


class Cells:
    """HemoCellFields: all membrane vertices on this GPU and the per-phase operations."""

    def __init__(self, lattice, P):
        self.lib = capi.lib()
        self.lattice = lattice
        self.P = P
        self.ptr = C.c_void_p()
        check(self.lib.hcp_create(C.byref(self.ptr), lattice.ptr, C.byref(P)))
        self.types = []
        self._next_id = 0
        self.rep_timescale = self.brep_timescale = 0   # cadences of the two repulsions (0 = off)

    def addCellType(self, celltype, material_timescale=1):
        idx = C.c_int()
        check(self.lib.hcp_add_type(self.ptr, celltype.ptr, int(material_timescale), C.byref(idx)))
        self.types.append(celltype)
        if getattr(celltype, "interior_viscosity", False):
            check(self.lib.hcp_type_set_interior_viscosity(self.ptr, idx.value, celltype.interiorViscosityTau))
        if getattr(celltype, "solidify", None) is not None:
            self.enableSolidifyMechanics(idx.value, *celltype.solidify)
        return idx.value

    # HemoCellField::kernelMethod (core/hemoCellField.h:67)
    def setIbmKernel(self, type_index, kernel):
        """the delta function of one type: IBM_PHI2 (the reference's interpolationCoefficientsPhi2, the default), IBM_PHI3
        (three-point, Roma) or IBM_PHI4 (four-point, Peskin); types of different widths share the container"""
        check(self.lib.hcp_type_set_ibm_kernel(self.ptr, int(type_index), int(kernel)))

    def ibmKernel(self, type_index):
        k = C.c_int()
        check(self.lib.hcp_type_get_ibm_kernel(self.ptr, int(type_index), C.byref(k)))
        return k.value

    # solidify mechanics (core/hemoCell.cpp:334-340; core/hemoCellParticleField.cpp:1002-1065)
    def enableSolidifyMechanics(self, type_index, distance_threshold_lu, shear_threshold):
        check(self.lib.hcp_type_set_solidify(self.ptr, int(type_index), float(distance_threshold_lu), float(shear_threshold)))

    def setSolidifyTimeScaleSeparation(self, n):
        """iterate() then runs prepareSolidification and solidifyCells every n iterations, before advanceParticles"""
        check(self.lib.hcp_set_solidify_timescale(self.ptr, int(n)))

    def prepareSolidification(self):
        """every complete cell of an enabled type with a flagged vertex turns its inner fluid nodes into wall nodes and
        binding sites, and leaves"""
        check(self.lib.hcp_solidify_prepare(self.ptr))

    def solidifyCells(self):
        """flags the vertices of enabled types that lie near a binding site under enough shear"""
        check(self.lib.hcp_solidify_flag(self.ptr))

    def solidifyFlags(self):
        """bool per vertex, in the order of positions"""
        out = np.empty(self.counts()[0], dtype=np.uint8)
        check(self.lib.hcp_solidify_flags_download(self.ptr, out.ctypes.data))
        return out.astype(bool)

    def setSolidifyFlags(self, flags):
        ff = np.ascontiguousarray(np.asarray(flags).astype(bool), dtype=np.uint8)
        if ff.shape != (self.counts()[0],):
            raise HcError("one flag per vertex: expected %d, got %s" % (self.counts()[0], ff.shape))
        check(self.lib.hcp_solidify_flags_upload(self.ptr, ff.ctypes.data))

    def solidify_counts(self):
        """(cells solidified, nodes solidified, vertices flagged now)"""
        o = (C.c_long * 3)()
        check(self.lib.hcp_solidify_counts(self.ptr, o))
        return tuple(int(v) for v in o)

    # interior viscosity (core/hemoCell.cpp:347-357, 404-410; core/hemoCellParticleField.cpp:745-807)
    def setInteriorViscosityTimeScaleSeparation(self, separation, separation_entire_grid):
        """iterate() then runs internalGridPointsMembrane every `separation` and deleteIncompleteCells +
        findInternalParticleGridPoints every `separation_entire_grid` iterations, after the constitutive model; both must be
        multiples of the velocity-update timescale"""
        check(self.lib.hcp_set_interior_timescales(self.ptr, int(separation), int(separation_entire_grid)))

    def findInternalParticleGridPoints(self):
        check(self.lib.hcp_interior_find(self.ptr))

    def internalGridPointsMembrane(self):
        check(self.lib.hcp_interior_membrane(self.ptr))

    def interiorPoints(self):
        """tau at the tagged nodes and 0 elsewhere, [nx][ny][nz] -- the reference's interiorViscosityField"""
        cls = self.lattice.interiorClasses()
        tau = np.r_[0.0, 1.0 / self.lattice.interiorViscosityOmegas()]
        return tau[cls]

    def interiorNormals(self, t):
        """the outward vertex normals the membrane pass would use now, [cells * nv][3] of type t"""
        f, n = self.type_range(t)
        out = np.empty((n * self.types[t].nv, 3), dtype=np.float64)
        check(self.lib.hcp_interior_normals(self.ptr, int(t), dptr(out)))
        return out

    def addCell(self, type_index, centre_lu, angles_deg=(0.0, 0.0, 0.0), min_dist_um=0.0, cell_id=None):
        """one line of a .pos file, already in lattice units; angles in degrees as in the file
        (io/readPositionsBloodCells.cpp:218-229: rad, then negated)"""
        c = np.array(centre_lu, dtype=np.float64)
        a = np.array(angles_deg, dtype=np.float64) * (3.14159265358979323846 / 180.0)
        a = a * -1.0
        placed = C.c_int()
        cid = self._next_id if cell_id is None else int(cell_id)
        self._next_id = max(self._next_id, cid + 1)
        check(self.lib.hcp_add_cell(self.ptr, int(type_index), cid, dptr(c), dptr(a), float(min_dist_um), C.byref(placed)))
        return bool(placed.value)

    def counts(self):
        nv, nc, nd = C.c_long(), C.c_long(), C.c_long()
        check(self.lib.hcp_counts(self.ptr, C.byref(nv), C.byref(nc), C.byref(nd)))
        return nv.value, nc.value, nd.value

    def type_range(self, t):
        f, n = C.c_long(), C.c_long()
        check(self.lib.hcp_type_range(self.ptr, int(t), C.byref(f), C.byref(n)))
        return f.value, n.value

    def _get(self, what):
        out = np.empty((self.counts()[0], 3), dtype=np.float64)
        check(self.lib.hcp_download(self.ptr, what, dptr(out)))
        return out

    def _set(self, what, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.counts()[0], 3):
            raise HcError("vertex array must have shape (%d, 3), got %s" % (self.counts()[0], a.shape))
        check(self.lib.hcp_upload(self.ptr, what, dptr(a)))

    positions = property(lambda s: s._get(0), lambda s, a: s._set(0, a))
    velocities = property(lambda s: s._get(1), lambda s, a: s._set(1, a))
    forces = property(lambda s: s._get(2), lambda s, a: s._set(2, a))

    def cell_ids(self):
        ids = np.empty(self.counts()[1], dtype=np.int64)
        check(self.lib.hcp_download_cell_ids(self.ptr, lptr(ids)))
        return ids

    # HemoCellParticle::serializeValues_t (core/hemoCellParticle.h:45-63), 120 bytes per vertex
    SV_DTYPE = np.dtype({"names": ["v", "position", "force", "force_repulsion", "cellId", "vertexId", "restime", "celltype"],
                         "formats": [("<f8", 3), ("<f8", 3), ("<f8", 3), ("<f8", 3), "<i8", "<u2", "<u4", "u1"],
                         "offsets": [0, 24, 48, 72, 96, 104, 108, 112], "itemsize": 120})

    def records(self):
        """every particle as the reference's particle record (removed particles of incomplete cells are not listed)"""
        rec = np.zeros(self.counts()[0] - self.deletion_counts()[3], dtype=self.SV_DTYPE)
        check(self.lib.hcp_download_records(self.ptr, rec.ctypes.data, len(rec)))
        return rec

    def set_records(self, rec):
        """replace the whole population by these records (any order, complete cells)"""
        rec = np.ascontiguousarray(rec, dtype=self.SV_DTYPE)
        check(self.lib.hcp_upload_records(self.ptr, rec.ctypes.data, len(rec)))

    def addVertexForce(self, vertex_index, f):
        idx = np.ascontiguousarray(vertex_index, dtype=np.int64)
        ff = np.ascontiguousarray(f, dtype=np.float64).reshape(len(idx), 3)
        check(self.lib.hcp_add_vertex_force(self.ptr, lptr(idx), len(idx), dptr(ff)))

    def vertex_stats(self, what=2):
        """ParticleInfo::calculate{Velocity,Force}Statistics: (min, max, mean, n) of |v| (what 1) or
        |force + force_repulsion| (what 2) over the owned vertices, reduced on the device"""
        o = np.zeros(3); n = C.c_long()
        check(self.lib.hcp_vertex_stats(self.ptr, int(what), dptr(o), C.byref(n)))
        return o[0], o[1], (o[2] / n.value if n.value else 0.0), n.value

    def setRepulsion(self, r_const, r_cutoff_um, timescale=1):
        """hemocell.setRepulsion(k, cutoff [um]) + setRepulsionTimeScaleSeperation(timescale)"""
        check(self.lib.hcp_set_repulsion(self.ptr, float(r_const), float(r_cutoff_um) * (1e-6 / self.P.dx), int(timescale)))
        self.rep_timescale = int(timescale)

    def applyRepulsionForce(self):
        check(self.lib.hcp_repulsion(self.ptr))

    def enableBoundaryParticles(self, br_const, br_cutoff_um, timescale=1):
        """hemocell.enableBoundaryParticles(k, cutoff [um], timestep) (core/hemoCell.cpp:428-436)"""
        check(self.lib.hcp_set_boundary_repulsion(self.ptr, float(br_const), float(br_cutoff_um) * (1e-6 / self.P.dx), int(timescale)))
        self.brep_timescale = int(timescale)

    def applyBoundaryRepulsionForce(self):
        check(self.lib.hcp_boundary_repulsion(self.ptr))

    @property
    def repulsion_forces(self):
        out = np.empty((self.counts()[0], 3), dtype=np.float64)
        check(self.lib.hcp_download_repulsion(self.ptr, dptr(out)))
        return out

    def spreadParticleForce(self, force_limit=True):
        check(self.lib.hcp_spread(self.ptr, int(force_limit)))

    def interpolateFluidVelocity(self):
        check(self.lib.hcp_interpolate(self.ptr))

    def advanceParticles(self, check_deletions=True):
        check(self.lib.hcp_advance(self.ptr, int(check_deletions)))

    # what happens to a particle that reaches a wall: the reference removes that single particle
    # (core/hemoCellParticleField.cpp:566-588, "particle", default) -- or the whole cell goes at once ("cell")
    def setDeletionMode(self, mode):
        check(self.lib.hcp_set_deletion_mode(self.ptr, {"particle": 0, "cell": 1}[mode]))

    def deleteIncompleteCells(self):
        """HemoCellFields::deleteIncompleteCells (core/hemoCellParticleField.cpp:512-553); returns the cells removed"""
        n = C.c_long()
        check(self.lib.hcp_delete_incomplete_cells(self.ptr, C.byref(n)))
        return n.value

    def deletion_counts(self):
        """(cells removed entirely, particles removed, incomplete cells listed now, their missing particles)"""
        a, b, c, d = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        check(self.lib.hcp_deletion_counts(self.ptr, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def alive(self):
        out = np.empty(self.counts()[0], dtype=np.uint8)
        check(self.lib.hcp_download_alive(self.ptr, out.ctypes.data))
        return out.astype(bool)

    def sampleScalar(self, scalar):
        """the scalar field's C at every vertex, through the interpolation stencil of interpolateFluidVelocity"""
        out = np.empty(self.counts()[0], dtype=np.float64)
        check(self.lib.hcp_sample_scalar(self.ptr, scalar.ptr, dptr(out)))
        return out

    def applyConstitutiveModel(self, iter_=0, forced=False):
        check(self.lib.hcp_mechanics(self.ptr, int(iter_), int(forced)))

    def force_components(self, t):
        f, n = self.type_range(t)
        nv = self.types[t].nv
        comp = np.empty((6, n * nv, 3), dtype=np.float64)
        check(self.lib.hcp_mechanics_components(self.ptr, int(t), dptr(comp)))
        return comp

    def cell_info(self, t):
        f, n = self.type_range(t)
        vol, area, bbox, cen = np.empty(n), np.empty(n), np.empty((n, 6)), np.empty((n, 3))
        check(self.lib.hcp_cell_info(self.ptr, int(t), dptr(vol), dptr(area), dptr(bbox), dptr(cen)))
        return dict(volume=vol, area=area, bbox=bbox, position=cen)

    def destroy(self):
        if self.ptr:
            check(self.lib.hcp_destroy(self.ptr))
            self.ptr = C.c_void_p()


class HemoCell:
    """hemo::HemoCell facade for one GPU (hemocell.h:68-253): owns lattice + cellfields, iterate()."""

    def __init__(self, lattice, P):
        self.lattice = lattice
        self.P = P
        self.cellfields = Cells(lattice, P)
        self.iter = 0
        self.particleVelocityUpdateTimescale = 1
        self.force_limit = True
        self.deletion_check_every = 1

    def setParticleVelocityUpdateTimeScaleSeparation(self, n):
        self.particleVelocityUpdateTimescale = int(n)

    def iterate(self, n=1):
        it = C.c_long(self.iter)
        check(capi.lib().hc_iterate(self.lattice.ptr, self.cellfields.ptr, C.byref(it), int(n),
                                    self.particleVelocityUpdateTimescale, int(self.force_limit),
                                    int(self.deletion_check_every)))
        self.iter = it.value

    def synchronize(self):
        check(capi.lib().hc_synchronize())


class Statistics:
    """Running statistics of a lattice and, for the cell sets, of one Cells container on it (hc_stats): sums kept on the
    device, sampled every `every` iterations inside iterate() -- the handle sits on the lattice, so every path that goes
    through hc_iterate or hc_preinlet_iterate honours it -- or by sample().  `what` is a mask of the sets below or an
    iterable of their names.  Arrays are fp64, in the lattice's node order z + nz*(y + ny*x).  Destroy the Statistics
    before its lattice and container."""
    RHO_U, UU, PI, CELL_DENSITY, INSIDE = 1, 2, 4, 8, 16
    SETS = {"rho_u": 1, "uu": 2, "pi": 4, "cell_density": 8, "inside": 16}

    def __init__(self, lattice, cells=None, what=RHO_U | UU | PI, every=0):
        self.lib = capi.lib()
        self.lattice, self.cells = lattice, cells
        if not isinstance(what, int):
            what = sum(self.SETS[str(w)] for w in set(what))
        self.what = int(what)
        self.ptr = C.c_void_p()
        check(self.lib.hc_stats_create(lattice.ptr, cells.ptr if cells is not None else None, self.what, C.byref(self.ptr)))
        if every:
            self.setEvery(every)

    def setEvery(self, every):
        """sample after every iteration it with (it + 1) % every == 0; 0: explicit samples only"""
        check(self.lib.hc_stats_set_every(self.ptr, int(every)))

    def sample(self):
        """one sample now, queued behind the work in flight; does not wait"""
        check(self.lib.hc_stats_sample(self.ptr))

    def reset(self):
        check(self.lib.hc_stats_reset(self.ptr))

    @property
    def samples(self):
        n = C.c_long()
        check(self.lib.hc_stats_samples(self.ptr, C.byref(n)))
        return n.value

    def sums(self, which):
        """the raw sums of one fluid set: [n][4] (rho, u) for RHO_U, [n][6] (xx, xy, xz, yy, yz, zz) for UU and PI"""
        which = self.SETS.get(which, which) if isinstance(which, str) else int(which)
        out = np.empty((self.lattice.n, 4 if which == self.RHO_U else 6), dtype=np.float64)
        check(self.lib.hc_stats_download_fluid(self.ptr, which, dptr(out)))
        return out

    def counts(self, which, type_index):
        """the raw int64 counts [n] of one cell set (CELL_DENSITY or INSIDE) and cell type"""
        which = self.SETS.get(which, which) if isinstance(which, str) else int(which)
        out = np.empty(self.lattice.n, dtype=np.int64)
        check(self.lib.hc_stats_download_cells(self.ptr, which, int(type_index), lptr(out)))
        return out

    def _mean(self, a):
        n = self.samples
        if n == 0:
            raise HcError("Statistics: no samples yet")
        return a / float(n)

    def mean_density(self):
        return self._mean(self.sums(self.RHO_U)[:, 0])

    def mean_velocity(self):
        return self._mean(self.sums(self.RHO_U)[:, 1:4])

    def velocity_covariance(self):
        """<u_a u_b> - <u_a><u_b>, [n][6] in the order xx, xy, xz, yy, yz, zz"""
        u = self.mean_velocity()
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        return self._mean(self.sums(self.UU)) - np.stack([u[:, a] * u[:, b] for a, b in pairs], axis=1)

    def mean_pi_neq(self):
        return self._mean(self.sums(self.PI))

    def cell_density(self, type_index):
        """mean number of vertices of the type whose nearest node this is"""
        return self._mean(self.counts(self.CELL_DENSITY, type_index).astype(np.float64))

    def hematocrit(self, type_index):
        """fraction of the samples in which the node lay inside a cell of the type (fluid nodes only; two cells that
        overlap on a node both count)"""
        return self._mean(self.counts(self.INSIDE, type_index).astype(np.float64))

    def destroy(self):
        if self.ptr:
            check(self.lib.hc_stats_destroy(self.ptr))
            self.ptr = C.c_void_p()


def pipe_mask(nx, ny, nz):
    """analytic cylinder along x replacing tube.stl: radius (ny-2)/2 centred at
    ((ny-1)/2,(nz-1)/2); node solid iff r > R"""
    y = np.arange(ny)[:, None] - (ny - 1) / 2.0
    z = np.arange(nz)[None, :] - (nz - 1) / 2.0
    R = (ny - 2) / 2.0
    solid = (y * y + z * z) > R * R
    return np.ascontiguousarray(np.broadcast_to(solid[None], (nx, ny, nz)).astype(np.uint8)), R
