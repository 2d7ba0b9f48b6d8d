/*
 * hemocell_amd.h -- C ABI of the MI355X-native IB-LBM hot path.
 *
 * Drop-in boundary for the one data-parallel path of HemoCell:
 * the D3Q19 Guo-BGK collide-stream, the phi2 immersed-boundary spread /
 * interpolate, the Euler vertex advance and the rbcHighOrderModel /
 * wbcHighOrderModel / rbcMalariaModel / pltSimpleModel membrane forces.  Every entry point names the reference
 * interface it replaces (file:line relative to the HemoCell tree).  Plain
 * pointers and sizes only; no C++/torch types cross this boundary.  All
 * functions return 0 on success and a non-zero code on failure, with the
 * message available from hc_last_error() (the reference logs and exit(1)s,
 * e.g. core/hemoCell.cpp:75-78; a library must not, so the host layer above
 * this ABI does that).  The library is HIP-only: there is no CPU fallback and
 * every call fails loudly when no gfx950 device is usable.
 *
 * Threading / process model: one process per GPU, one hc_* context per process
 * (core/hemoCell.cpp:75-79 has the same rule).
 */
#ifndef HEMOCELL_AMD_H
#define HEMOCELL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HC_OK 0
#define HC_ERR_HIP 1
#define HC_ERR_ARG 2
#define HC_ERR_STATE 3

#define HC_Q 19

typedef struct hc_lattice hc_lattice;   /* one x-slab of the D3Q19 lattice on this GPU          */
typedef struct hc_celltype hc_celltype; /* CommonCellConstants + moduli of one cell type         */
typedef struct hc_cells hc_cells;       /* all membrane vertices held by this GPU (SoA)          */

/* ------------------------------------------------------------------ runtime */
const char *hc_last_error(void);
/* selects the HIP device, checks it is gfx950; replaces plb::plbInit (core/hemoCell.cpp:80-86).  A multi-rank run passes
 * its LOCAL rank modulo hc_device_count (one process per GPU); hc_comm_init_env does that by itself. */
int hc_init(int device);
int hc_device_count(int *count);
/* run every kernel of this library on an existing hipStream_t (e.g. the host framework's current stream); NULL = library stream */
int hc_set_stream(void *hip_stream);
int hc_synchronize(void);
/* fork-join onto a second stream owned by the library, for phase-by-phase callers (slab runs) that want what
 * hc_iterate does on its own: hc_fork() makes the side stream wait for everything enqueued so far, hc_route(1) sends the
 * launches of the following calls there (hc_route(0): back to the main stream), hc_join() makes the main stream wait
 * for them.  Between two velocity updates advance, mechanics and the next spread run beside the collide this way. */
int hc_fork(void);
int hc_route(int side);
int hc_join(void);
int hc_side_stream(void **hip_stream);  /* the side stream's hipStream_t, for a host framework that has to enqueue its own work (transfers) there */
/* hc_iterate overlaps those phases by itself (default); 0 = strictly one stream (A/B measurements) */
int hc_set_overlap(int on);
/* per-launch hipEvent timing of the dominant kernel (helper/profiler.h:46-77 "collideAndStream" timer) */
int hc_profile_enable(int on);
int hc_profile_read(const char *kernel, double *total_ms, long *launches); /* "collide_stream" (every launch) = "collide_stream_alone" + "collide_stream_beside" (launches with advance / spread on the side stream next to them), "ibm_spread", "ibm_interpolate", "advance", "mechanics", "lees_edwards" (both kernels of the pass), "collide_stream_interior" (how many of the "collide_stream" launches ran the interior-viscosity instantiation: a count, its time is 0), "interior_find", "interior_membrane" (one entry per pass), "stats_fluid", "stats_cell_density", "stats_inside" (the kernels of one hc_stats sample; the two cell kernels once per cell type) */
int hc_profile_reset(void);
/* identifies the build of the dominant kernel: first 16 hex digits of the SHA-256 of csrc/lattice.hip and csrc/d3q19.h (a committed PMC
 * traffic figure is only quoted next to a timing when it was measured on the same kernel) */
const char *hc_build_tag(void);
/* device-to-device copy of `bytes` on the library stream, `repeats` times: read + written GB/s of the GPU in hand */
int hc_measure_copy_bandwidth(size_t bytes, int repeats, double *gbytes_per_s);
/* Reproducible force spreading.  The reference adds the particles' forces to the lattice particle by particle, in storage
 * order (core/hemoCellParticleField.cpp:841-863): a run repeats bit for bit.  The default kernels here add with fp64 atomics in
 * whatever order the hardware takes them, so two runs of one input differ in the last bits.  on = 1 selects the gather form:
 * every (particle, stencil node) contribution is keyed by its node, sorted stably in (cell type, cell id, vertex id) order and
 * summed by one thread per node -- identical bits from run to run and from one slab decomposition to another, at several times
 * the cost of the atomic kernel.  Also selected by HEMOCELL_REPRODUCIBLE_SPREAD=1 in the environment. */
int hc_set_reproducible_spread(int on);
/* A/B switch: 1 = per-vertex IBM kernels with direct global atomics instead of the LDS-tiled per-cell kernels */
int hc_debug_ibm_per_vertex(int on);
int hc_debug_force_plane_padding(int on); /* tests / A-B runs: lattices created afterwards get the padded x-plane stride whatever their size (1), never (-1), by size (0, default) */

/* ---------------------------------------------------------------- ranks (one process per GPU of one node)
 * Replaces what plb::plbInit / MPI give the reference (core/hemoCell.cpp:80-86, the MPI calls of SURVEY.md section 2.3):
 * a rank, a world size and neighbour exchange.  Two layers:
 *   control plane  a TCP mesh between the ranks (loopback / MASTER_ADDR): bootstrap, barrier, reductions of a few
 *                  scalars at output cadence, agreement on the placed cells.  Never on the stepping path.
 *   data plane     HC_TRANSPORT_RCCL: ncclSend / ncclRecv between x-neighbours, grouped, on the library's side stream
 *                  (RCCL over xGMI; /opt/rocm/lib/librccl.so.1 is loaded on demand); HC_TRANSPORT_TCP: the same messages
 *                  staged through pinned host memory and the mesh -- for ranks that SHARE a GPU (RCCL refuses two ranks
 *                  on one device), i.e. rehearsals and tests on a one-GPU box.
 * hc_comm_init_env reads RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT (torch.distributed.run's names; also
 * OMPI_COMM_WORLD_RANK / _SIZE / _LOCAL_RANK and PMI_RANK / PMI_SIZE of an mpirun), HEMOCELL_PORT (default MASTER_PORT + 1017)
 * and HEMOCELL_TRANSPORT = rccl | tcp (unset: HC_TRANSPORT_AUTO), selects the device LOCAL_RANK modulo the device count (hc_init) and
 * connects.  Without those variables it is a one-rank world and does nothing. */
#define HC_TRANSPORT_NONE 0
#define HC_TRANSPORT_RCCL 1
#define HC_TRANSPORT_TCP 2
#define HC_TRANSPORT_AUTO 3   /* RCCL when every rank can set it up and a ring self-test completes; otherwise TCP, announced on stderr */
int hc_comm_init_env(void);
/* explicit form; init_device != 0: also hc_init(local_rank % device count).  transport HC_TRANSPORT_NONE builds the control
 * plane only (host-side use without a GPU: the CPU tests of the mesh). */
int hc_comm_init(int rank, int world, int local_rank, const char *master_addr, int port, int transport, int init_device);
int hc_comm_finalize(void);
int hc_comm_info(int *rank, int *world, int *transport);
int hc_comm_barrier(void);
/* v[n] <- reduction over all ranks, folded in rank order on rank 0 (deterministic); op: 0 sum, 1 min, 2 max */
int hc_comm_allreduce(double *v, int n, int op);
int hc_comm_bcast(void *buf, size_t bytes, int root);
/* all[r * bytes ..] <- rank r's block, on every rank (the reference's HemoCellGatheringFunctional, core/hemoCellFunctional.h:101-112) */
int hc_comm_allgather(const void *mine, size_t bytes, void *all);
/* neighbour exchange of HOST buffers over the control plane with the same routing rule as the data plane (my low-face
 * message is the low neighbour's high-halo message; the ring closes when periodic != 0): what the CPU tests check */
int hc_comm_exchange_host(int periodic, const void *send_lo, size_t n_lo, const void *send_hi, size_t n_hi,
                          void *recv_lo, size_t m_lo, void *recv_hi, size_t m_hi);
/* counters of the slab schedule since the last reset (reset != 0 clears them): out[0..7] = envelope records sent, new
 * copies created, copies dropped, cells deleted at a wall, iterations, host seconds spent enqueueing them, host seconds
 * waiting for the id headers, velocity-update steps */
int hc_slab_stats(hc_lattice *L, double out[8], int reset);

/* ------------------------------------------------------------------ lattice */
/* MultiBlockLattice3D<T,DESCRIPTOR>(nx,ny,nz, new GuoExternalForceBGKdynamics(omega))
 * (examples/pipeflow/pipeflow.cpp:66-71).  nx is the LOCAL slab thickness;
 * x-halos of width 2 are allocated on both sides.  periodic[0] with
 * n_slabs==1 wraps in-kernel; with n_slabs>1 the caller exchanges halos
 * (hcl_halo_pack / hcl_halo_unpack).  x0 = global x of local plane 0. */
int hcl_create(hc_lattice **out, int nx, int ny, int nz, const int periodic[3], double omega,
               int x0, int nx_global, int n_slabs);
int hcl_destroy(hc_lattice *L);
/* defineDynamics(lattice, flagMatrix, bbox, new BounceBack(1.), 0) (examples/pipeflow/pipeflow.cpp:73):
 * mask[node]=1 -> full-way bounce-back / isBoundary (3..6: moving wall classes, see hcl_set_wall_velocity); node = z + nz*(y + ny*x_local), x_local in [-2, nx+2)
 * i.e. the array holds (nx+4)*ny*nz bytes including the halo planes. */
int hcl_set_mask(hc_lattice *L, const uint8_t *mask_with_halo);
/* HemoCell::latticeEquilibrium(rho,u) + lattice->initialize() (core/hemoCell.cpp:129-133) */
int hcl_init_equilibrium(hc_lattice *L, double rho, const double u[3]);
/* setExternalVector(lattice, bbox, forceBeginsAt, F) (core/hemoCell.cpp:369-371, examples/pipeflow/pipeflow.cpp:144-146):
 * the uniform driving force; the per-node IBM force is kept separately and zeroed by the collide kernel */
int hcl_set_body_force(hc_lattice *L, const double F[3]);
/* setExternalVector on PART of the domain (cases/kolmogorovFlow/kolmogorovFlow.cpp:136-140: +F on one half of the box, -F on
 * the other): n <= HC_MAX_FORCE_REGIONS boxes, boxes[k] = {x0, x1, y0, y1, z0, z1} inclusive GLOBAL node ranges, whose nodes
 * carry forces[k] instead of the uniform body force; where boxes overlap the later one holds, as with consecutive
 * setExternalVector calls.  n = 0 removes them.  Evaluated inside the kernels from these few numbers: no force field in HBM. */
#define HC_MAX_FORCE_REGIONS 4
int hcl_set_body_force_regions(hc_lattice *L, int n, const int *boxes, const double *forces);
/* setBoundaryVelocity(lattice, box, u) on nodes flagged by setVelocityConditionOnBlockBoundaries
 * (helper/hemocellInit.hh:71-86): mask classes 3..6 are moving no-slip walls with velocity u (full-way
 * bounce-back + Ladd momentum term; stand-in for Palabos' regularised boundary, which is not available) */
int hcl_set_wall_velocity(hc_lattice *L, int wall_class, const double u[3]);
/* lattice->collideAndStream() (core/hemoCell.cpp:317), n times (fluid-only stepping).  On a slab of a multi-rank run
 * (n_slabs > 1, hc_comm_init* done) the faces are exchanged inside, interior planes colliding meanwhile. */
int hcl_collide_stream(hc_lattice *L, int nsteps);
/* Lees-Edwards shear boundary on the two z faces (helper/leesEdwardsBC.h).  After every step of hcl_collide_stream and
 * hc_iterate (after hcl_step_end, before the interpolation) the top layer z = nz-1 and the bottom layer z = 0 of the
 * post-stream state are replaced: collideExternal(rhoBar, j = (v, 0, 0)) on a copy of each node, then five populations
 * interpolated between the nodes s1, s2 of the same layer shifted by the displacement D along x.  Needs n_slabs = 1, a
 * lattice periodic on all three axes, nz >= 4 and fluid nodes only in the layers z = 0, 1, nz-2, nz-1 (a later hcl_set_mask
 * that breaks this is refused).  Enabling sets D = 0 and no schedule. */
int hcl_set_lees_edwards(hc_lattice *L, double v_top, double v_bottom);
/* the displacement the next pass uses.  d_per_iteration != 0: hc_iterate sets D = fmod(d * (it + 1), nx) after the step that
 * ends at iteration it + 1 (LeesEdwardsBC::updateLECurDisplacement after every HemoCell::iterate); hcl_collide_stream never
 * changes D */
int hcl_set_lees_edwards_displacement(hc_lattice *L, double D, double d_per_iteration);
/* one pass on the current state (Palabos' lattice->initialize() runs the integrated processors once) */
int hcl_lees_edwards_apply(hc_lattice *L);
/* out = {D, v_top, v_bottom, d_per_iteration} */
int hcl_lees_edwards_state(const hc_lattice *L, double out[4]);
/* Zou-He open boundaries, here with normal x (Palabos' addVelocityBoundary0N/0P, addPressureBoundary0N/0P).  kind: HC_OB_VELOCITY
 * (u given, rho from the known populations) or HC_OB_PRESSURE (rho given, u = (u_x, 0, 0) from them); orientation -1 = 0N
 * (the populations with c_x = +1 are completed), +1 = 0P (c_x = -1).  The completion runs inside the collide, between the
 * gather and the Guo-forced BGK, on the post-stream populations of the declared nodes; their mask stays fluid, and nodes
 * that are bounce-back stay bounce-back.  nodes: [n][3] local node coordinates; the nodes get the consecutive slots
 * first_slot .. first_slot + n - 1, starting at u = 0 and rho = 1.  A node holds one slot: a call that names a node that
 * is an open-boundary node already, or names a node twice, is refused and changes nothing (hcl_open_boundary_clear removes
 * all).  While a lattice has such nodes, every observer (hcl_download_rho_u, hcl_download_pi_neq, hcl_plane_velocity,
 * the velocity statistic of hcl_fluid_stats (what 0), the IBM interpolation) takes its moments of the COMPLETED populations
 * of a fluid open-boundary node: a velocity node reports u_bc + F / 2, a pressure node its prescribed density.  The force
 * and mass statistics (what 1, 2) are untouched: mass is the sum of the STORED populations, which is what is conserved.  Lattices without open boundaries run the
 * collide and the observers exactly as before.  Needs a lattice without a Lees-Edwards boundary (and
 * hcl_set_lees_edwards refuses a lattice with open-boundary nodes): the two do not combine.
 * On a slab of a multi-rank run (n_slabs > 1, ranks connected -- an unconnected lattice takes open boundaries with n_slabs = 1
 * only) every rank declares the nodes of its own slab, in LOCAL coordinates and with slots of its own; a node outside the slab
 * is "node outside the lattice".  Nodes of any axis may lie on a slab's face planes, x-normal ones also on a plane that has a
 * neighbour.  The slab schedule and the observers then give the single domain's bits, and the face-velocity message
 * (hcl_face_velocity_pack) carries completed moments for the open nodes of a face plane. */
#define HC_OB_VELOCITY 0
#define HC_OB_PRESSURE 1
int hcl_open_boundary_add(hc_lattice *L, int kind, int orientation, const int *nodes, int n, int *first_slot);
/* every node of the inclusive local box {x0, x1, y0, y1, z0, z1}, x outermost and z innermost */
int hcl_open_boundary_add_box(hc_lattice *L, int kind, int orientation, const int box[6], int *first_slot, int *n_nodes);
/* The same with the normal along any axis: axis 0, 1 or 2 (x, y, z; anything else is HC_ERR_ARG) -- Palabos'
 * addVelocityBoundary1N ... addPressureBoundary2P.  orientation -1 completes the populations with c_axis = +1, +1 those with
 * c_axis = -1.  The completion on axis a is the x completion with the roles of x and a exchanged: the normal velocity is
 * u[a], a pressure node takes the prescribed rho, the normal velocity from the known populations and tangential velocity 0.
 * The values of a slot stay {u_x, u_y, u_z, rho} in lattice axes whatever the axis.  Every rule above holds unchanged (one
 * slot per node, on whatever axis it was declared; local coordinates on a slab; no Lees-Edwards; bounce-back nodes stay bounce-back), and
 * so do the observers.  Nodes where two open faces meet get no dynamics of their own: they are the caller's to make walls.
 * hcl_open_boundary_add and _add_box are these with axis 0.  A lattice holds fewer than 2^27 open-boundary nodes. */
int hcl_open_boundary_add_axis(hc_lattice *L, int kind, int axis, int orientation, const int *nodes, int n, int *first_slot);
int hcl_open_boundary_add_box_axis(hc_lattice *L, int kind, int axis, int orientation, const int box[6], int *first_slot, int *n_nodes);
int hcl_open_boundary_clear(hc_lattice *L);
/* slots[i] = the slot of local node nodes[i], or -1 */
int hcl_open_boundary_slots(const hc_lattice *L, const int *nodes, int n, int *slots);
/* axes[i] = the axis (0, 1, 2) on which local node nodes[i] was declared, or -1 */
int hcl_open_boundary_axes(const hc_lattice *L, const int *nodes, int n, int *axes);
/* setBoundaryVelocity / setBoundaryDensity on slots first_slot .. first_slot + n - 1: u [n][3], rho [n], read from the
 * device (on_device != 0, ordered on the library's stream) or from the host */
int hcl_open_boundary_set_velocity(hc_lattice *L, int first_slot, int n, const double *u, int on_device);
int hcl_open_boundary_set_density(hc_lattice *L, int first_slot, int n, const double *rho, int on_device);
/* out = [n][4] {u_x, u_y, u_z, rho} of the slots, host */
int hcl_open_boundary_values(hc_lattice *L, int first_slot, int n, double *out);
/* Cell::computeVelocity on nodes of the plane x of the post-stream state: u = j/rho + F/2 with F the body force (and the
 * force regions) alone -- what HemoCell's force field holds after iterate() and setExternalVector.  yz: [n] in-plane
 * indices y * nz + z (host); out: [n][3] on the device (on_device != 0, ordered on the library's stream) or the host.
 * Bounce-back nodes give 0.  Needs n_slabs = 1.  It is hcl_plane_velocity_axis with axis 0. */
int hcl_plane_velocity(hc_lattice *L, int x, const int *yz, int n, double *out, int on_device);
/* The same on the plane coordinate[axis] == plane of any axis (0, 1, 2; x local, 0 .. nx - 1).  idx: [n] in-plane indices, the
 * node's offset with the axis removed and the remaining axes in lattice order: y * nz + z (axis 0), x * nz + z (axis 1),
 * x * ny + y (axis 2).  Every rule above holds (n_slabs = 1, bounce-back nodes give 0, a lattice with open-boundary nodes
 * reports completed moments, also on a plane that lies on or crosses an open face).  Another axis, a plane outside the
 * lattice or an index outside the plane is HC_ERR_ARG.  The node list is staged from the host and the call ends in a wait
 * for the library's stream: it is an observer, not a per-iteration path (that is hcl_preinlet_apply). */
int hcl_plane_velocity_axis(hc_lattice *L, int axis, int plane, const int *idx, int n, double *out, int on_device);
/* The pre-inlet's fluid coupling kept on the device (helper/preInlet.cpp, applyPreInletVelocityBoundary): the plane velocities
 * of the lattice `pre` on its plane coordinate[axis] == pre_plane at the in-plane indices pre_idx[0 .. n-1] (as for
 * hcl_plane_velocity_axis) become the velocities of the domain's open-boundary slots domain_first_slot .. + n - 1, node k
 * to slot domain_first_slot + k.  create uploads the index list once and checks: n_slabs = 1 on the pre-inlet lattice, and on
 * the domain too unless axis == 0 (a slab domain: the inlet plane of an x direction lies on one rank, the slots are that
 * rank's local slots and the handle lives in that rank's process beside its own pre-inlet lattice; a y or z plane would span
 * the ranks), plane and indices in range, the slots exist on the domain and every one of them is a velocity slot (else HC_ERR_ARG).  The handle
 * holds plain pointers to both lattices and owns neither: destroy it BEFORE either lattice.
 * apply: one kernel on the library's stream, no staging, no copy and no host wait; it writes u_x, u_y, u_z of the slots and
 * leaves rho alone.  It reads the domain's slot storage and the pre-inlet's state at the time of the call, so slots
 * declared on the domain after create (which may move that storage) do no harm.  After hcl_open_boundary_clear on the
 * domain the coupled slots are gone: apply and iterate then return HC_ERR_STATE and launch nothing, also when nodes were
 * declared again since -- make a new handle.
 * iterate: n times (hcl_collide_stream(pre, 1), hcl_collide_stream(domain, 1), apply), the reference's per-iteration order,
 * all queued on the library's stream without a host wait: the domain lags the pre-inlet by one iteration.  With a slab
 * domain the domain's step is COLLECTIVE: the other ranks call hcl_collide_stream(domain, ...) or hc_iterate for the same
 * number of steps, or the face exchange inside waits for them until the transport's timeout. */
typedef struct hc_preinlet hc_preinlet;
int hcl_preinlet_create(hc_preinlet **out, hc_lattice *pre, hc_lattice *domain, int axis, int pre_plane,
                        const int *pre_idx, int n, int domain_first_slot);
int hcl_preinlet_apply(hc_preinlet *P);
int hcl_preinlet_iterate(hc_preinlet *P, int n);
int hcl_preinlet_destroy(hc_preinlet *P);
/* bring the x-halo planes of a slab up to date (width 1 or 2, see hcl_halo_doubles) through the data plane; the
 * download / statistics entry points do it by themselves */
int hcl_slab_refresh_halos(hc_lattice *L, int width);
/* one collide-stream of this slab; halos must be current. part: 0 = all planes, 1 = interior planes
 * (those that do not read halo data), 2 = the two face planes; or 3 = planes 2..nx-3, 4 = the two planes next to each
 * face (what the node velocities of a face plane are evaluated from, hcl_face_velocity_pack, so that the messages of a velocity
 * update can travel while part 3 runs).
 * hcl_step_end() flips the buffers. */
int hcl_collide_stream_part(hc_lattice *L, int part);
/* parts 5 and 6: as 2 and 4, but the halo planes of the IBM force buffer being retired are left for the caller to clear with
 * hcl_zero_force_halos (before hcl_step_end) -- the slab schedule sends its face message first */
int hcl_zero_force_halos(hc_lattice *L);
int hcl_step_end(hc_lattice *L);
/* populations in the reference's own layout: AoS [node][19], node = z + nz*(y + ny*x), values f_i - t_i
 * as Palabos stores them (post-stream state, i.e. what Cell::operator[] returns after collideAndStream) */
int hcl_download_populations(hc_lattice *L, double *f_aos);
int hcl_upload_populations(hc_lattice *L, const double *f_aos);   /* on a slab of a multi-rank run: collective (the ranks exchange their face planes) */
/* rho[n] and u[n][3] = Cell::computeVelocity (j/rho + F/2), local bulk nodes */
int hcl_download_rho_u(hc_lattice *L, double *rho, double *u);
/* pi[n][6] = the off-equilibrium momentum flux of the post-stream populations (xx, xy, xz, yy, yz, zz), the quantity
 * Cell::computeShearStress and computeStrainRateFromStress scale (io/FluidHdf5IO.hh:419-443, :497-552), local bulk nodes */
int hcl_download_pi_neq(hc_lattice *L, double *pi);
/* IBM force field currently accumulated (without the body force), [node][3] */
/* FluidInfo::calculate{Velocity,Force}Statistics (helper/fluidInfo.cpp:33-118) as a device reduction: out = {min, max,
 * sum} of the magnitude over the non-boundary bulk nodes of this slab, *n_nodes their number.  what: 0 =
 * Cell::computeVelocity, 1 = external force (body force + the IBM field spread for the coming step), 2 = rhoBar (sum of
 * the 19 stored populations) over ALL bulk nodes, walls included: its sum is the conserved mass.  Deterministic. */
int hcl_fluid_stats(hc_lattice *L, int what, double out[3], long *n_nodes);
int hcl_download_ibm_force(hc_lattice *L, double *F);
int hcl_zero_ibm_force(hc_lattice *L);
/* halo exchange (Palabos duplicateOverlaps(staticVariables), core/hemoCell.cpp:142).  width = 1 (5
 * populations per face, enough for one collide-stream) or 2 (needed before an IBM interpolation: the 14
 * populations of the face plane that do not move away from the neighbour and, from the plane behind it, the 5
 * that stream onto the neighbour's first halo plane).  side 0 = low-x face, 1 = high-x face.  Buffers are DEVICE pointers of
 * hcl_halo_doubles(L,width) doubles each. */
size_t hcl_halo_doubles(const hc_lattice *L, int width);
int hcl_halo_pack(hc_lattice *L, int side, int width, double *dev_buf);
int hcl_halo_unpack(hc_lattice *L, int side, int width, const double *dev_buf);
/* as hcl_halo_pack, but from the buffer the collide-stream in progress is writing (between
 * hcl_collide_stream_part(L, 4) and hcl_step_end): lets the message leave before the interior planes are done */
int hcl_halo_pack_next(hc_lattice *L, int side, int width, double *dev_buf);
/* the width-1 message of BOTH faces in one launch (what hc_iterate uses every step; a null buffer = no neighbour on that side);
 * next != 0: from the buffer the collide in progress is writing */
int hcl_halo_pack_both(hc_lattice *L, double *dev_lo, double *dev_hi, int next);
int hcl_halo_unpack_both(hc_lattice *L, const double *dev_lo, const double *dev_hi);
/* the message of a velocity update between slabs: node velocities u = j/rho + F/2 (Cell::computeVelocity for
 * ExternalForceDynamics, what core/hemoCellParticleField.cpp:833 blends) of this slab's face plane `side`, evaluated by
 * their owner on the post-stream state and packed as [3][ny*nz] doubles (device pointer) for the neighbour whose first halo
 * plane it is -- 3 planes instead of the 19 population planes of a width-2 halo.  hc_iterate exchanges them itself.
 * On a lattice with open-boundary nodes a fluid open node of the plane sends the moments of its completed populations (a
 * velocity node u_bc + F / 2), as every observer reports them; bounce-back nodes send 0. */
int hcl_face_velocity_pack(hc_lattice *L, int side, double *dev_buf);
int hcl_face_velocity_pack_both(hc_lattice *L, double *dev_lo, double *dev_hi);   /* both face planes in one launch; a null buffer = no neighbour there */
int hcl_download_face_velocity(hc_lattice *L, int side, double *host_u /*[3][ny*nz]*/);   /* the same plane on the host, for inspection */
int hcl_dims(const hc_lattice *L, int dims[3]);
/* counts[0] = bulk nodes of this slab, [1] = fluid nodes (GuoExternalForceBGKdynamics), [2] = nodes the collide kernel
 * loads and stores (everything but solid nodes without a fluid neighbour, which full-way bounce-back leaves inert) */
int hcl_node_counts(const hc_lattice *L, long counts[3]);
double hcl_mlups_bytes_per_node(const hc_lattice *L); /* algorithmic bytes per node update of the collide kernel */
/* Interior viscosity (INTERIOR_VISCOSITY builds of the reference: core/hemoCellField.cpp:100-112 clones the background
 * dynamics with omega = 1 / tau_int for nodes inside a cell, attributeDynamics in core/hemoCellParticleField.cpp:745-807).
 * Here a node carries one class byte: 0 relaxes with the lattice's omega, k >= 1 with omega[k - 1]; the dynamics are the
 * same Guo-forced BGK otherwise.  The field is allocated by the first hcl_interior_enable (all 0) and from then on the collide
 * runs an instantiation of its own that loads the byte next to the mask byte; a lattice that never enables it runs the
 * kernels it always ran.  A second call replaces the omegas and keeps the field.  Refused (HC_ERR_ARG, with a message):
 * n_slabs > 1, a lattice with open-boundary nodes or a Lees-Edwards boundary -- and the open-boundary, Lees-Edwards and
 * pre-inlet calls refuse a lattice that has it enabled, so the order of the calls does not matter.
 * classes: uint8 [nx][ny][nz] in the bulk numbering z + nz * (y + ny * x); upload refuses a class above n_classes.  This pair
 * is also how a checkpoint carries the field.  The passes that maintain it from the cells are hcp_interior_find and
 * hcp_interior_membrane. */
#define HC_MAX_VISC_CLASSES 7
int hcl_interior_enable(hc_lattice *L, int n_classes, const double *omega /*[n_classes]*/);
int hcl_interior_info(const hc_lattice *L, int *n_classes /* 0: not enabled */, double *omega /*[HC_MAX_VISC_CLASSES] or NULL*/);
int hcl_interior_upload_classes(hc_lattice *L, const uint8_t *classes);
int hcl_interior_download_classes(hc_lattice *L, uint8_t *classes);

/* The CEPAC field (core/hemoCellFields.cpp:120-133): a passive scalar, a dissolved agonist concentration C, on a D3Q19
 * advection-diffusion lattice bound to one hc_lattice, which carries it.  The reference leaves the field half finished and its
 * fluid library is not part of its tree, so this back end defines the step itself (csrc/scalar.hip states it operation by
 * operation, tests/scalar_ref.py restates it; DESIGN.md section 6 lists the deviations):
 *   fluid node   g_i <- g_i (1 - omega) + omega t_i (Cbar + 3 C c_i.u), Cbar = sum g_i, C = 1 + Cbar, diffusivity (1/omega - 1/2)/3
 *   wall node    full-way bounce-back: zero scalar flux, no momentum term for moving walls
 *   source node  every population is set to t_i (C_s - 1 + 3 C_s c_i.u); observers report C_s there
 * u is the flow's velocity after the collide-stream of the same iteration: j/rho of the post-stream populations plus half of the
 * body and IBM force that collide consumed -- hcl_scalar_step belongs after hcl_step_end.  hc_iterate runs one step per
 * iteration there, before the interpolation (core/hemoCell.cpp:320-325); hcl_collide_stream alone does not step the scalar.
 * Refused (HC_ERR_ARG, with a message): omega outside (0,2); n_slabs > 1; a lattice with open-boundary nodes, a Lees-Edwards
 * boundary, interior viscosity or a pre-inlet handle (hcl_preinlet_create / hcp_preinlet_create*), and those calls refuse a
 * lattice that has a scalar; a second scalar on one lattice.  hcl_destroy destroys the lattice's scalar with it.
 * A new field holds C = 1.  box: inclusive node ranges {x0, x1, y0, y1, z0, z1}, clipped to the lattice; NULL = every node.
 * Sources: at most HC_MAX_SCALAR_SOURCES distinct values on the lattice at a time (a value whose nodes were all painted over
 * gives its slot back); a box that would bring one more, or a value that is not a number, is refused and changes nothing; a
 * box wholly outside the lattice registers nothing.
 * Arrays are in the bulk numbering z + nz * (y + ny * x): C_out [n], populations [n][19] in the visible post-stream convention
 * of hcl_download_populations, u_out [n][3] (0 on nodes that are not fluid), out3 = {sum, minimum, maximum} of C over the
 * fluid nodes.  hcp_sample_scalar: C at every vertex through the IBM interpolation stencil (fluid nodes only, weights
 * renormalised), in the vertex order of hcp_download; removed vertices give 0. */
typedef struct hc_scalar hc_scalar;
#define HC_MAX_SCALAR_SOURCES 8
int hcl_scalar_create(hc_lattice *L, double omega, hc_scalar **out);
int hcl_scalar_destroy(hc_scalar *S);
int hcl_scalar_init_equilibrium(hc_scalar *S, const int box[6] /* or NULL */, double C);
int hcl_scalar_set_source_box(hc_scalar *S, const int box[6], double C);
int hcl_scalar_clear_sources(hc_scalar *S);
int hcl_scalar_step(hc_scalar *S);
int hcl_scalar_download(hc_scalar *S, double *C_out);
int hcl_scalar_download_populations(hc_scalar *S, double *g_aos);
int hcl_scalar_upload_populations(hc_scalar *S, const double *g_aos);
int hcl_scalar_download_velocity(hc_scalar *S, double *u_out);
int hcl_scalar_stats(hc_scalar *S, double out3[3]);
int hcp_sample_scalar(hc_cells *C, hc_scalar *S, double *out_per_vertex);

/* --------------------------------------------------------------- cell types */
#define HC_MODEL_RBC_HO 0     /* mechanics/rbcHighOrderModel.cpp */
#define HC_MODEL_PLT_SIMPLE 1 /* mechanics/pltSimpleModel.cpp    */
#define HC_MODEL_WBC_HO 2     /* mechanics/wbcHighOrderModel.cpp: hcp_celltype_create_wbc or _ex */
#define HC_MODEL_RBC_MALARIA 3 /* mechanics/rbcMalariaModel.cpp: hcp_celltype_create_ex */
#define HC_SHAPE_WBC_SPHERE 0            /* config/constant_defaults.h:83 */
#define HC_SHAPE_RBC_FROM_SPHERE 1       /* config/constant_defaults.h:80 */
#define HC_SHAPE_MESH_FROM_STL 2         /* config/constant_defaults.h:84: hcp_celltype_create_ex */
#define HC_SHAPE_ELLIPSOID_FROM_SPHERE 6 /* config/constant_defaults.h:81 */

typedef struct hc_params { /* Parameters::lbm_base_parameters, mechanics/constantConversion.cpp:36-59 */
  double dx, dt, nu_p, rho_p, kBT_p;
  double tau, nu_lbm, dm, df, f_limit, kBT_lbm;
} hc_params;
int hc_params_base(hc_params *P, double dx, double dt, double nu_p, double rho_p, double kBT_p);

typedef struct hc_material { /* <MaterialModel> of RBC.xml / PLT.xml */
  double kLink, kArea, kVolume, kBend, eta_m;
  double radius;       /* [m] */
  int min_triangles;
  double aspect_ratio; /* ellipsoid only */
  const long *inner_edges; /* [n_inner][2] (PLT.xml:14-38) or NULL */
  int n_inner;
} hc_material;

/* hemocell.addCellType<Model>(name, constructType) (hemocell.h:122-128): builds the mesh
 * (helper/meshGeneratingFunctions.hh), CommonCellConstants (mechanics/commonCellConstants.cpp:70-409) and
 * the moduli (mechanics/cellMechanics.h:50-78), and uploads the tables. */
int hcp_celltype_create(hc_celltype **out, int model, int shape, const hc_params *P, const hc_material *M);

/* the extra <MaterialModel> tags of WBC_HO.xml (mechanics/wbcHighOrderModel.cpp:242-262), SI units */
typedef struct hc_wbc_material {
  double kInnerRigid;   /* [N]  rigid-core inner-link modulus */
  double kCytoskeleton; /* [N]  cytoskeleton inner-link modulus */
  double coreRadius;    /* [m] */
  double radius;        /* [m]  cell radius of the cytoskeleton law (the same tag as hc_material.radius in the XML) */
} hc_wbc_material;
/* hemocell.addCellType<WbcHighOrderModel>(name, constructType): the RBC_HO moduli of M plus the inner-link law over
 * M->inner_edges (wbcHighOrderModel.cpp:199-223).  hcp_celltype_create refuses HC_MODEL_WBC_HO and names this entry point. */
int hcp_celltype_create_wbc(hc_celltype **out, int shape, const hc_params *P, const hc_material *M, const hc_wbc_material *W);
/* lattice-unit WBC constants: out = k_inner_rigid, k_cytoskeleton, core_radius, radius (0 for the other models) */
int hcp_celltype_wbc_constants(const hc_celltype *T, double out[4]);

/* everything hemocell.addCellType<Model>(name, constructType) reads from a cell XML, for any model and construct type */
typedef struct hc_celltype_spec {
  int model;                  /* HC_MODEL_* */
  int shape;                  /* HC_SHAPE_* */
  hc_material material;       /* min_triangles is not read for HC_SHAPE_MESH_FROM_STL */
  const hc_wbc_material *wbc; /* HC_MODEL_WBC_HO only, else NULL */
  double kInnerLink;          /* HC_MODEL_RBC_MALARIA only: <kInnerLink>, in kBT per persistence length (may be 0) */
  const char *stl_path;       /* HC_SHAPE_MESH_FROM_STL only: <StlFile>, binary or ASCII STL, opened as given */
} hc_celltype_spec;
/* the general creation call: accepts every model x shape pair.  MESH_FROM_STL follows constructCell
 * (helper/meshGeneratingFunctions.hh:275-288): largest bounding-box extent scaled to 2 radius, rotate_zxz(pi/2, pi/2, 0),
 * centre 0, vertices welded by first occurrence on exact coordinates, inflated 1e-3 along the vertex normals.  A missing
 * file, an open or non-manifold mesh and a degenerate triangle are refused.  RBC_MALARIA is the RBC_HO model with the
 * membrane viscosity always evaluated plus the linear inner links of mechanics/rbcMalariaModel.cpp:198-217. */
int hcp_celltype_create_ex(hc_celltype **out, const hc_params *P, const hc_celltype_spec *S);
/* lattice-unit malaria constant: out[0] = k_inner_link (mechanics/rbcMalariaModel.cpp:233-240; 0 for the other models) */
int hcp_celltype_malaria_constants(const hc_celltype *T, double out[1]);
int hcp_celltype_destroy(hc_celltype *T);
/* table sizes: out[0..3] = vertices, triangles, edges, inner edges */
int hcp_celltype_sizes(const hc_celltype *T, int out[4]);
/* host copies of the tables for inspection / output writers; any pointer may be NULL */
int hcp_celltype_tables(const hc_celltype *T, double *vertices /*[nv][3]*/, long *triangles /*[nt][3]*/,
                        long *edges /*[ne][2]*/, double *edge_length_eq, double *edge_angle_eq,
                        double *triangle_area_eq, long *vertex_vertexes /*[nv][6]*/, double *patch_dist_eq,
                        double scalars[9] /* volume_eq, area_mean_eq, edge_mean_eq, angle_mean_eq, k_volume, k_area, k_link, k_bend, eta_m */);

/* the remaining CommonCellConstants tables (mechanics/commonCellConstants.h:64-85); any pointer may be NULL */
int hcp_celltype_tables2(const hc_celltype *T, long *edge_bending_triangles /*[ne][2]*/, long *edge_bending_outer_points /*[ne][2]*/,
                         long *inner_edges /*[nie][2]*/, double *inner_edge_length_eq /*[nie]*/, int *vertex_n_vertexes /*[nv]*/);

/* ---------------------------------------------------------------- cells */
/* HemoCellFields / HemoCellParticleField (core/hemoCellFields.h:103-158, core/hemoCellParticleField.h:39-207) */
int hcp_create(hc_cells **out, hc_lattice *L, const hc_params *P);
int hcp_destroy(hc_cells *C);
int hcp_add_type(hc_cells *C, hc_celltype *T, int material_timescale /* setMaterialTimeScaleSeparation */, int *type_index);
/* loadParticles() (io/readPositionsBloodCells.cpp:290-361) for one cell: centre in lattice units (GLOBAL
 * coordinates), angles in radians, already negated as :228-229 does.  placed=0 when a vertex falls on /
 * within min_dist_um of a boundary node (:139-164) and the cell is dropped.
 * On a slab (n_slabs > 1) every rank offers every cell: the call keeps it when one of its particles has its nearest node in
 * this slab or it reaches within the envelope of a face (periodic images are tried shifted by +-nx_global,
 * core/hemoCellParticleDataTransfer.cpp:33-65), placed=0 otherwise; a rank sees the wall only next to its slab, so
 * hcp_slab_sync_placement must follow the last cell: it drops on every rank the cells any rank rejected and reports how
 * many distinct cells of each type the whole domain now holds. */
int hcp_add_cell(hc_cells *C, int type, long cell_id, const double centre_lu[3], const double angles[3],
                 double min_dist_um, int *placed);
/* slot for a cell whose state is restored afterwards with hcp_upload (checkpoint resume,
 * core/hemoCellFields.cpp:240-275): undeformed mesh at centre_lu, no wall test */
int hcp_add_cell_unchecked(hc_cells *C, int type, long cell_id, const double centre_lu[3], const double angles[3]);
/* n_vertices counts the listed vertices (cells x vertices per cell; an incomplete cell keeps its slots), n_deleted the
 * cells removed entirely so far */
int hcp_slab_sync_placement(hc_cells *C, long *global_cells_per_type /*[n types]*/);
/* The particle envelope of a slab run: <particleEnvelope> of the case configuration in lattice units
 * (examples/pipeflow/config.xml:34), read at core/hemoCell.cpp:139 and handed to HemoCellFields (core/hemoCellFields.cpp:39-43).
 * The reference replicates single particles within that distance of a block face on the neighbour; here whole cells are
 * replicated, so an envelope E acts as share = E - (diameter of the largest cell type): how far a cell may still travel
 * towards the face, between two velocity updates, before a complete copy must exist on the other side (default share: 4 lu).
 * Call after the cell types are added and before the first cell is placed.  A request the slab width cannot support
 * (nx >= 2 * diameter + 2 * share) is clamped and the share in use returned; a slab too thin for the minimum (2 lu) is an
 * error.  Every copy that arrives late -- a particle already within reach of the receiving slab's nodes when its cell first
 * gets there -- is counted on the device (hcp_envelope) and fails the hc_iterate call that notices it. */
int hcp_set_envelope(hc_cells *C, double particle_envelope_lu, double *share_in_use);
int hcp_envelope(const hc_cells *C, double *share_in_use, long *late_copies);
int hcp_counts(hc_cells *C, long *n_vertices, long *n_cells, long *n_deleted);
int hcp_type_range(hc_cells *C, int type, long *first_vertex, long *n_cells);
/* What happens to a particle whose nearest node is a boundary after advance (core/hemoCellParticleField.cpp:566-588):
 *   HC_DELETE_PARTICLE (default, the reference): removeParticles(1) takes that particle out (:304-321); its cell is
 *     incomplete from then on -- no mechanics (:634-652), forces of the remaining particles zeroed at the next material
 *     step (:660-667), still spread / interpolated / advanced -- until hcp_delete_incomplete_cells removes the rest
 *     (deleteIncompleteCells, :512-553: the reference calls it at every writeOutput, core/hemoCell.cpp:248-252, and at
 *     velocity-update steps when verbose.cellsDeletedInfo is set, :361-363);
 *   HC_DELETE_CELL: the whole cell goes at once.
 * Either way the decision is taken on the device inside the advance kernel and costs no host round trip; slab runs
 * (n_slabs > 1) remove an incomplete cell on all its holders at the next velocity update, i.e. behave as the reference
 * with cellsDeletedInfo. */
#define HC_DELETE_PARTICLE 0
#define HC_DELETE_CELL 1
int hcp_set_deletion_mode(hc_cells *C, int mode);
int hcp_delete_incomplete_cells(hc_cells *C, long *n_cells_removed);
/* cells removed entirely / single particles removed so far; incomplete cells and missing particles currently listed */
int hcp_deletion_counts(hc_cells *C, long *cells_removed, long *particles_removed, long *incomplete_cells, long *missing_particles);
/* alive[i] = 0 for a removed particle of an incomplete cell, in hcp_download order */
int hcp_download_alive(hc_cells *C, unsigned char *alive);
/* serializeValues_t fields as [n][3] arrays in cell-major order; what: 0 position 1 velocity 2 force */
int hcp_download(hc_cells *C, int what, double *out);
int hcp_upload(hc_cells *C, int what, const double *in);
int hcp_download_cell_ids(hc_cells *C, long *ids);
/* The same state in the reference's own particle record, HemoCellParticle::serializeValues_t (core/hemoCellParticle.h:45-63,
 * 120 bytes: v @0, position @24, force @48, force_repulsion @72, plint cellId @96, uint16 vertexId @104, uint restime @108,
 * uchar celltype @112), so that a binding can hand over the contents of libhemocell's std::vector<HemoCellParticle>:
 * download writes one record per vertex (n_records = hcp_counts vertices; types, cells, vertices in order);
 * upload replaces the whole population by the given records, in any order, every cell complete. */
int hcp_download_records(hc_cells *C, void *records, long n_records);
int hcp_upload_records(hc_cells *C, const void *records, long n_records);
/* HemoCellStretch::ForceForcedLsps (helper/hemoCellStretch.cpp:63-78): sv.force += f on listed vertices.  vertex_index
 * counts vertices in hcp_download order at the time of the call (cells deleted by the last hc_iterate are not counted).
 * The result is bit for bit that of `force[vertex_index[i]] += f[i]` for i = 0 .. n-1 in list order, also when a vertex
 * is listed more than once; an index outside [0, number of vertices) refuses the whole call and changes nothing. */
int hcp_add_vertex_force(hc_cells *C, const long *vertex_index, int n, const double *f /*[n][3]*/);
/* hemocell.setRepulsion(k, cutoff) + setRepulsionTimeScaleSeperation (core/hemoCell.cpp:394-397,420-426); the
 * cutoff is given in lattice units (the facade converts from micrometres).  hc_iterate then evaluates
 * cellfields->applyRepulsionForce() (core/hemoCell.cpp:307-309 -> core/hemoCellParticleField.cpp:677-743) every
 * `timescale` iterations; spread adds force_repulsion + force as the reference does. */
/* ParticleInfo::calculate{Velocity,Force}Statistics (helper/particleInfo.cpp:30-140) as a device reduction over the
 * vertices this slab owns: out = {min, max, sum} of |v| (what 1) or |force + force_repulsion| (what 2). */
int hcp_vertex_stats(hc_cells *C, int what, double out[3], long *n);
int hcp_set_repulsion(hc_cells *C, double r_const, double r_cutoff_lu, int timescale);
int hcp_repulsion(hc_cells *C);
int hcp_download_repulsion(hc_cells *C, double *out /*[n][3]*/);
/* hemocell.enableBoundaryParticles(k, cutoff, timestep) (core/hemoCell.cpp:428-436): wall nodes with a non-wall node
 * among their 26 neighbours (populateBoundaryParticles, core/hemoCellParticleField.cpp:865-890) push the vertices
 * binned around them; hcp_boundary_repulsion is cellfields->applyBoundaryRepulsionForce() (core/hemoCell.cpp:310-312 ->
 * core/hemoCellParticleField.cpp:891-918) and ADDS to force_repulsion, which only hcp_repulsion resets (:703).
 * hc_iterate applies it every `timescale` iterations.  Call after hcl_set_mask. */
int hcp_set_boundary_repulsion(hc_cells *C, double br_const, double br_cutoff_lu, int timescale);
int hcp_boundary_repulsion(hc_cells *C);
/* cellfields->spreadParticleForce() (core/hemoCell.cpp:313 -> core/hemoCellParticleField.cpp:841-863) */
int hcp_spread(hc_cells *C, int force_limit);
/* cellfields->interpolateFluidVelocity() (core/hemoCell.cpp:329 -> core/hemoCellParticleField.cpp:819-839) */
int hcp_interpolate(hc_cells *C);
/* the same for the listed cells of one type only (slab runs interpolate the cells that cross a face first, so that
 * their records travel while the rest is interpolated) */
int hcp_interpolate_cells(hc_cells *C, int type, const int *slots, int n);
/* cellfields->advanceParticles() (core/hemoCell.cpp:342 -> core/hemoCellParticleField.cpp:566-588) */
int hcp_advance(hc_cells *C, int check_deletions);
/* cellfields->applyConstitutiveModel(forced) (core/hemoCell.cpp:345 -> core/hemoCellParticleField.cpp:633-675) */
int hcp_mechanics(hc_cells *C, long iter, int forced);
/* separate_force_vectors output mode (core/hemoCellParticleField.cpp:590-614): comp = [6][n][3]
 * (volume, area, bending, link, visc, inner link) for the vertices of one type */
int hcp_mechanics_components(hc_cells *C, int type, double *comp);
/* ---- the width of a type's IBM delta function (HemoCellField::kernelMethod, core/hemoCellField.h:67).  The reference declares
 * phi3, phi4, interpolationCoefficientsPhi3 and ...Phi4 (core/immersedBoundaryMethod.h:43-50, :140-153) without bodies; the
 * definitions here are this back end's own, the standard three-point (Roma) and four-point (Peskin) functions:
 *   phi3(r) = (1 + sqrt(1 - 3 r^2)) / 3 for |r| <= 0.5, (5 - 3 |r| - sqrt(-2 + 6 |r| - 3 r^2)) / 6 for 0.5 < |r| <= 1.5, else 0;
 *     nodes c - 1, c, c + 1 per axis with c = floor(p + 0.5)
 *   phi4(r) = (3 - 2 |r| + sqrt(1 + 4 |r| - 4 r^2)) / 8 for |r| <= 1, (5 - 2 |r| - sqrt(-7 + 12 |r| - 4 r^2)) / 8 for 1 < |r| <= 2, else 0;
 *     nodes f - 1 ... f + 2 per axis with f = floor(p)
 * Everything else is interpolationCoefficientsPhi2 (:99-137): weight = phi(dx) phi(dy) phi(dz), nodes in ascending x, y, z, a
 * node beyond a non-periodic face, a node that is not fluid and a zero weight skipped, the admitted weights times 1 / total.
 * hcp_spread, hcp_interpolate, hcp_interpolate_cells and hc_iterate then run the type through the kernels of that width, in
 * all three forms (per cell, per vertex, reproducible spread); types of different widths share a container.  A cell whose
 * stencil nodes exceed the tile or node cap of its width takes the per-vertex path inside the per-cell kernels.
 * HC_ERR_ARG, and nothing changes: another value of `kernel`; a wide kernel on a lattice with n_slabs > 1 (four points need two
 * halo planes), with open-boundary nodes or in a pre-inlet pair, or for a type with interior viscosity (the membrane pass walks
 * the eight-node stencil).  The other way round, hcl_open_boundary_add*, hcl_preinlet_create, hcp_preinlet_create*,
 * hcp_type_set_interior_viscosity and hcp_sample_scalar refuse while a type of the container (a container of the lattice) is
 * on a wide kernel.  Default HC_IBM_PHI2, which launches exactly what it launched before this call existed. */
#define HC_IBM_PHI2 2
#define HC_IBM_PHI3 3
#define HC_IBM_PHI4 4
int hcp_type_set_ibm_kernel(hc_cells *C, int type, int kernel);
int hcp_type_get_ibm_kernel(hc_cells *C, int type, int *kernel);
/* ---- interior viscosity: which nodes lie inside a cell (core/hemoCellParticleField.cpp:745-807, helper/octree.h:107-147,
 * helper/mollerTrumbore.h).  hcp_type_set_interior_viscosity marks a type (<enableInteriorViscosity>, tau_int =
 * viscosityRatio (tau - 0.5) + 0.5): omega = 1 / tau_int becomes a class of the lattice (an equal omega shares a class;
 * hcl_interior_enable is called as needed); a type is marked once -- the same tau_int again changes nothing, another one is HC_ERR_ARG.  Only HC_MODEL_RBC_HO carries a normal in the reference; any other model,
 * more than HC_MAX_VISC_CLASSES distinct omegas and everything hcl_interior_enable refuses are HC_ERR_ARG.
 * hcp_interior_find (findInternalParticleGridPoints): clears the class field, then for every complete cell of a marked
 * type tests every integer node of the truncated bounding box of its (unwrapped) vertices: the node is interior when the
 * number of triangles the ray from the node along (-40, -40, -40) hits is odd, helper/mollerTrumbore.h operation for
 * operation.  The node is wrapped onto the lattice as the IBM stencil wraps (periodic axes) or dropped (outside a
 * non-periodic axis), and tagged with the type's class when it is a fluid node.  Where cells of several classes overlap,
 * the cell with the highest id wins.  The caller removes incomplete cells first (hcp_delete_incomplete_cells), as
 * core/hemoCell.cpp:348 does; cells that still are incomplete are skipped.
 * hcp_interior_membrane (internalGridPointsMembrane): for every live vertex of a marked type, every admitted node of its
 * phi2 stencil (non-zero weight, fluid) no farther than edge_mean_eq from the vertex is tagged when (node - position) . n < 0
 * and cleared otherwise; n is the vertex's outward normal, the sum over its triangles in ascending order of unit normal *
 * area / area_mean_eq (mechanics/rbcHighOrderModel.cpp:115-121), formed from the CURRENT positions; an incomplete cell's
 * vertices have n = 0 and so clear their nodes, as in the reference.  The result is that of visiting the vertices one after
 * the other in ascending (cell id, vertex index) order, the later one overruling the earlier, whatever the launch geometry.
 * Both passes are stream ordered, wait for nothing and write the class field: never beside a collide.
 * hcp_set_interior_timescales (setInteriorViscosityTimeScaleSeperation): hc_iterate then runs, after hcp_mechanics of an
 * iteration `it`, hcp_delete_incomplete_cells + hcp_interior_find when it % entire_grid_every == 0 and
 * hcp_interior_membrane when it % membrane_every == 0 (core/hemoCell.cpp:347-357); both must be multiples of hc_iterate's
 * particle_timescale (HC_ERR_ARG otherwise, core/hemoCell.cpp:614-620), which keeps such an iteration off the side stream.
 * Defaults 1, 1.  hcp_interior_normals: the normals the membrane pass would use now, [cells * nv][3] of one type. */
int hcp_type_set_interior_viscosity(hc_cells *C, int type, double tau_int);
int hcp_set_interior_timescales(hc_cells *C, int membrane_every, int entire_grid_every);
int hcp_interior_find(hc_cells *C);
int hcp_interior_membrane(hc_cells *C);
int hcp_interior_normals(hc_cells *C, int type, double *out);
/* tests: the workgroup size of the two passes (64, 128, 256 or 512; default 256) -- the class field does not depend on it */
int hc_debug_interior_block(int threads);
/* ---- solidify mechanics (SOLIDIFY_MECHANICS builds of the reference: core/hemoCellParticleField.cpp:920-1065,
 * mechanics/pltSimpleModel.cpp:211-252): platelets that come near a binding site on the wall, under enough shear, turn into
 * wall nodes, and those nodes become binding sites.
 * The binding field is one byte per node, 1 = a binding site, allocated (all 0) by the first hcl_binding_* call that writes.
 * hcl_binding_populate (populateBindingSites): every boundary node (mask != 0) of the inclusive box (x0, x1, y0, y1, z0, z1),
 * clipped to the lattice, with a fluid node among its 26 neighbours becomes a site; calls add up.  The neighbours wrap on
 * periodic axes and are dropped beyond a non-periodic end.  hcl_binding_download / _upload move the field as [nx][ny][nz]
 * bytes (a checkpoint carries it that way), hcl_binding_clear zeroes it.  hcl_download_mask: the mask classes the device
 * holds now, [nx][ny][nz], nodes solidified since hcl_set_mask included.
 * hcl_download_tresca (eigenValueFromCell): (lambda_max - lambda_min) / 2 of S = -omega * 3 / (2 rho) * PiNeq on fluid
 * nodes, PiNeq and rho as hcl_download_pi_neq and hcl_download_rho_u report them; 0 on every other node.  Formed with the
 * lattice's one omega: refused on slabs, with open boundaries and with interior viscosity.
 * hcp_type_set_solidify (enableSolidifyMechanics + <distanceThreshold>, <shearThreshold> of the type's <MaterialModel>; the
 * distance in lattice units): only HC_MODEL_PLT_SIMPLE, thresholds >= 0.  From then on every vertex carries a flag byte (0 for
 * new vertices), moved by hcp_solidify_flags_download / _upload in the vertex order of hcp_download.
 * hcp_solidify_prepare (prepareSolidification): every complete cell of an enabled type with a flagged vertex turns the fluid
 * nodes inside it (the ray cast of hcp_interior_find) into bounce-back nodes and binding sites, populations untouched, and
 * leaves like a cell that reached a wall.  hcp_solidify_flag (solidifyCells): a live vertex of an enabled type is flagged
 * when a binding site among its nearest node n = floor(pos + 0.5) and the 26 around it lies within the distance threshold
 * and |tresca(n) / 1e-7| exceeds the shear threshold; set flags stay set.  Both end by bringing the lattice's host mask up to
 * date (one host wait).  hc_iterate runs prepare, then flag, without a host wait, between hcp_interpolate and hcp_advance of
 * every iteration `it` with it % every == 0 (hcp_set_solidify_timescale, default 1; core/hemoCell.cpp:334-340), and refreshes
 * the host mask once before it returns.  hcp_solidify_counts: {cells solidified, nodes solidified, vertices flagged now};
 * solidified cells do not count in hcp_counts' n_deleted.  While a type is enabled, hcp_remove_cells and hcp_unpack_cells (the slot
 * moves of the slab exchange, which do not carry the flags) are refused on that container.
 * Refused (HC_ERR_ARG from these calls, HC_ERR_STATE from hc_iterate when the other feature came second): n_slabs > 1, open
 * boundaries, a Lees-Edwards boundary, interior viscosity, a pre-inlet.  A CEPAC field is fine: its step reads the flow's
 * mask, so a node that turns to wall bounces the scalar back from the next step on. */
int hcl_binding_populate(hc_lattice *L, const int box[6]);
int hcl_binding_clear(hc_lattice *L);
int hcl_binding_download(hc_lattice *L, uint8_t *out);
int hcl_binding_upload(hc_lattice *L, const uint8_t *in);
int hcl_download_mask(hc_lattice *L, uint8_t *out);
int hcl_download_tresca(hc_lattice *L, double *out);
/* a checkpoint's way back: every node with in[node] != 0 ([nx][ny][nz]) that is fluid now becomes a bounce-back node exactly as
 * hcp_solidify_prepare leaves it (class 1, populations untouched, wall-brick byte set, host mask refreshed) */
int hcl_upload_solidified_mask(hc_lattice *L, const uint8_t *in);
int hcp_type_set_solidify(hc_cells *C, int type, double distance_threshold_lu, double shear_threshold);
int hcp_set_solidify_timescale(hc_cells *C, int every);
int hcp_solidify_prepare(hc_cells *C);
int hcp_solidify_flag(hc_cells *C);
int hcp_solidify_flags_download(hc_cells *C, unsigned char *out);
int hcp_solidify_flags_upload(hc_cells *C, const unsigned char *in);
int hcp_solidify_counts(hc_cells *C, long out[3]);
/* tests: the workgroup size of the prepare pass (64, 128, 256 or 512; default 256) -- the result does not depend on it */
int hc_debug_solidify_block(int threads);
/* HemoCell::iterate() (core/hemoCell.cpp:299-376) n times, followed each time by the driver's body-force
 * re-application (examples/pipeflow/pipeflow.cpp:144-146).  particle_timescale =
 * setParticleVelocityUpdateTimeScaleSeparation. iter is read and advanced.  Particles that reach a wall are deleted on
 * the device at EVERY iteration (hcp_set_deletion_mode); deletion_check_every is only how often the host looks, without
 * waiting, whether storage can be compacted.  On a slab of a multi-rank run (n_slabs > 1) the same call runs the slab
 * schedule: faces of the 5 crossing populations every step and the particle envelopes at every velocity update
 * (syncEnvelopes, core/hemoCellFields.cpp:377-499) travel over the data plane beside the interior collide. */
int hc_iterate(hc_lattice *L, hc_cells *C, long *iter, int n, int particle_timescale, int force_limit,
               int deletion_check_every);
/* ---- multi-slab particle envelopes: HemoCellFields::syncEnvelopes (core/hemoCellFields.cpp:377-499) and
 * HemoCellParticleDataTransfer::send/receive (core/hemoCellParticleDataTransfer.cpp:33-180).  The host
 * decides WHICH cells cross a slab face (from hcp_cell_extents); the records move device-to-device.
 * A record is 9 doubles per vertex: position, velocity, force (the mutable part of serializeValues_t,
 * core/hemoCellParticle.h:45-63); x_shift is the periodic offset (+-nx_global) of :33-65. */
int hcp_cell_extents(hc_cells *C, int type, double *ext /*[n_cells][3] = min x, max x, #vertices whose nearest node is in this slab*/);
/* asynchronous form: _begin enqueues the kernel and the copy into pinned staging and returns; _end waits for that copy
 * only (an event), not for work enqueued afterwards, so the extents can be started early in a step and picked up
 * without draining the stream.  The cell set must not change in between. */
int hcp_cell_extents_begin(hc_cells *C, int type);
int hcp_cell_extents_end(hc_cells *C, int type, double *ext);
size_t hcp_record_doubles(const hc_cells *C, int type); /* doubles per cell record */
int hcp_pack_cells(hc_cells *C, int type, const int *slots, int n, double x_shift, double *dev_buf);
/* merge rule of HemoCellParticleField::addParticle (core/hemoCellParticleField.cpp:173-235): a local vertex
 * (nearest node in this slab) is kept, any other is overwritten; is_new cells are appended (slots must be
 * n_cells, n_cells+1, ... in order) */
int hcp_unpack_cells(hc_cells *C, int type, const int *slots, const long *cell_ids, const int *is_new, int n,
                     const double *dev_buf);
/* deleteNonLocalParticles (core/hemoCellFields.cpp:676-688) at cell granularity; holes are filled from the tail */
int hcp_remove_cells(hc_cells *C, int type, const int *slots, int n);
int hcp_owned_vertices(hc_cells *C, long *n_owned); /* vertices whose nearest node lies in this slab */

/* ---- the pre-inlet's cells (helper/preInlet.cpp:254-351, applyPreInletParticleBoundary; the offsets of
 * core/hemoCellParticleDataTransfer.cpp:33-65, 229-260).  Positions are kept unwrapped, so a cell of the periodic pre-inlet `pre`
 * that went `lap` times round its Lp nodes along `axis` sits at lap * Lp + (its place in the box): with cmin, cmax its extent
 * on the axis, lap = floor(cmin / Lp), and the cell is a candidate when it is complete and lies wholly in the window,
 * cmin - lap * Lp >= window_lo and cmax - lap * Lp <= window_hi.  A candidate arrives in `domain` at p + shift, on the axis at
 * p + (shift[axis] - lap * Lp), with the id id + (lap - orientation) * id_stride (orientation -1: a *neg direction, +1: *pos;
 * the offset of getOffset, positive for *neg), its velocity, force and force_repulsion copied, complete and alive.  Recorded
 * deviation: the reference copies single particles and deletes partly arrived cells later; here a cell is added only when
 * its id is absent and its WHOLE vertex set lies in the window -- partly arrived cells are never added.
 * create checks and refuses (HC_ERR_ARG, nothing launched): n_slabs = 1 on both lattices, the pre-inlet periodic on the axis,
 * the same number of cell types with the same model and vertex count, a repulsion on both containers or on neither,
 * 0 <= window_lo < window_hi <= Lp, id_stride > 0.  Not checked: the window must be wider than the largest cell plus the
 * distance travelled between two checks, or cells pass uninjected; the handle holds plain pointers to both containers and
 * is destroyed BEFORE either.
 * set_sink: with on != 0, every apply first removes (hcp_remove_cells) the domain's cells with cmax > plane (orientation -1)
 * or cmin < plane (+1) on the axis.
 * apply, on the library's stream: settles both containers, runs one select kernel per type and container, waits for that
 * kernel alone (an event -- the one host wait of a check), runs the sink, then offers the candidates in ascending (type,
 * slot) order: one whose new id this handle offered before is skipped; one whose shifted extents leave [0, n - 1] of the
 * domain on any axis is skipped and counted rejected; one whose new id the domain holds is skipped; the rest are appended
 * (slots n_cells, n_cells + 1, ...; within capacity without a copy through the host, as hcp_unpack_cells) and copied by one
 * kernel, slot to slot.
 * counts: out = {cells injected, rejected, removed by the sink, checks} since create.
 * hc_preinlet_iterate: n times (hc_iterate(pre, 1), hc_iterate(domain, 1), hcl_preinlet_apply(F), and hcp_preinlet_apply(X)
 * when the advanced iter is a multiple of cells_every >= 1), the reference driver's order; both systems share iter.
 *
 * A domain cut into x-slabs: hcp_preinlet_create_slab is COLLECTIVE -- every rank of the domain's world calls it with its own
 * slab's container and the same axis (0 only), orientation, window, shift and id_stride; shift and the sink plane are in global
 * domain coordinates.  The pre-inlet lives whole (n_slabs = 1) on the rank that holds the inlet plane (rank 0 for -1, the last
 * rank for +1), which passes its container as `pre`; every other rank passes null.  Refused on every rank (HC_ERR_ARG, the
 * refusing rank's message) when any rank refuses: an axis other than 0, a domain periodic along x, `pre` on the wrong rank or
 * missing on the inlet rank, what create refuses about the pair, arguments that differ between ranks, and a window whose
 * image [window_lo + shift[0], window_hi + shift[0]] does not lie in the inlet rank's slab at least the particle envelope
 * (hcp_envelope) away from that slab's inner face -- an arriving cell is then held by the inlet rank alone, none of its
 * vertices has a stencil node on the neighbour, and the ordinary envelope synchronisation replicates it later.
 * set_sink (the same arguments on every rank), apply, counts and destroy take the slab handle; on it apply is collective:
 * the one-domain rule on the global domain.  One host wait (the select kernels; the domain's counts the vertices each slab
 * owns), then at most two rounds over the control plane, none of which is skipped by a rank that failed locally -- it
 * says so in the round and every rank returns the error, with no container changed and the handle's counts and its memory
 * of what was offered as they were.  Round 1: the ranks that own part of a
 * cell past the sink plane name it, the inlet rank names its candidates (offered for the first time, shifted extents inside
 * the global box; the others count as rejected).  Round 2 (skipped when there is no sink and no candidate): every rank
 * names the candidates whose id it will still hold after the sink.  Then every holder, owner or pure copy, removes the
 * sink's cells -- in this check, before the next spread -- and the inlet rank appends the candidates nobody holds.  A
 * holder whose own select disagrees with the owners about a cell it holds returns HC_ERR_STATE through round 2.  After a
 * change to a type the extents already taken for the next envelope synchronisation are discarded.  n_injected, n_removed and
 * counts are totals of distinct cells over the whole domain, the same on every rank.
 * hc_preinlet_iterate with a slab handle: F is the inlet rank's fluid coupling and null on every other rank (null F with any
 * other handle is HC_ERR_ARG); the inlet rank steps the pre-inlet, its slab and applies F, the other ranks step their slabs,
 * and every cells_every iterations all ranks run the check together. */
typedef struct hc_preinlet_cells hc_preinlet_cells;
int hcp_preinlet_create(hc_preinlet_cells **out, hc_cells *pre, hc_cells *domain, int axis, int orientation /* -1: *neg, +1: *pos */,
                        double window_lo, double window_hi, const double shift[3], long id_stride);
int hcp_preinlet_create_slab(hc_preinlet_cells **out, hc_cells *pre /* null off the inlet rank */, hc_cells *domain, int axis, int orientation,
                             double window_lo, double window_hi, const double shift[3], long id_stride);
int hcp_preinlet_set_sink(hc_preinlet_cells *X, int on, double plane);
int hcp_preinlet_apply(hc_preinlet_cells *X, long *n_injected, long *n_removed);
int hcp_preinlet_counts(const hc_preinlet_cells *X, long out[4]);   /* injected, rejected, removed by the sink, checks */
int hcp_preinlet_destroy(hc_preinlet_cells *X);
int hc_preinlet_iterate(hc_preinlet *F, hc_preinlet_cells *X, long *iter, int n, int particle_timescale, int force_limit,
                        int deletion_check_every, int cells_every);

/* CellInformationFunctionals (helper/cellInfo.cpp:39-80,140-180): per cell volume, area, bbox[6], centroid[3].  For a cell that
 * lost particles at a wall (not yet deleteIncompleteCells'd) bbox and centroid cover the particles left (CellPosition);
 * volume and area are the triangle sums at the stored positions. */
int hcp_cell_info(hc_cells *C, int type, double *volume, double *area, double *bbox, double *centroid);

/* ------------------------------------------------------------------ packing
 * tools/packCells of the reference (packing.h, ellipsoid.h, geometry.h): Bargiel's force-biased packing of ellipsoids in a
 * periodic box with the Perram-Wertheim contact function.  Lengths are in grid cells: the box is grid[0] x grid[1] x grid[2],
 * sizes are the full axes of each species' enclosing ellipsoid already multiplied by the sizing factor (initBlood,
 * packing.h:198-262).  Particles are numbered species by species.  The caller supplies the initial state (the library draws
 * nothing): pos [N][3] inside the box, quat [N][4] = (s, p) or null for identity.  create runs Packing::init and the
 * calc_forces before the first iteration (:265-343, :179-182); ntau <= 0 and epsilon <= 0 take the reference's 102400 and
 * 0.1.  Refused (HC_ERR_ARG): a null pointer, a grid outside 1..1023 per axis, no particle in total, a negative count, a
 * non-positive size, anything non-finite, a position outside the box.
 * hc_packing_run queues up to max_steps more iterations (iterate, :345-368) and waits once; every kernel returns at once
 * after the end, so a run past it changes nothing.  status = { steps done in total, finished, Douter, Dinner, Pactual,
 * DensityNominal, Force_step, Relax, Nsf, error flag, largest root-search count, grow }.  The root search (zeroin, :697-764)
 * is capped at 256 evaluations: a pair that reaches the cap contributes nothing, sets the sticky error flag and this and every
 * later run returns HC_ERR_STATE.  grow = 1: a partner list was too short; the run stopped in front of that iteration's forces
 * with fewer steps done, the storage has grown, and the next run completes the iteration first.  max_steps < 0 is HC_ERR_ARG.
 * hc_packing_state: positions, quaternions, forces and torques in particle order (any pointer may be null).
 * hc_packing_pairs is a probe of the pair function the step uses (Packing::calc_forces(e, ei, ej), :108-144) on n given
 * pairs: sizes [n][3], quaternions [n][4] as Quaternion(s, p) takes them (it normalises), rij = pos_B - pos_A [n][3],
 * douter2 [n].  Out: lambda, 4 f_AB(lambda), n [n][3], the force and torque increments of A and B [n][3] each, the number of
 * evaluations of the root search and kind (0: nothing, lambda < 1e-10; 1: f_AB >= 1; 2: overlap; -1: the cap). */
typedef struct hc_packing hc_packing;
int hc_packing_create(hc_packing **out, const int grid[3], int n_species, const double *sizes, const int *counts, const double *pos,
                      const double *quat, double nominal_density, int rotate, int ntau, double epsilon);
int hc_packing_run(hc_packing *P, int max_steps, double status[12]);
int hc_packing_count(const hc_packing *P, int *n_particles, int *list_capacity);
int hc_packing_state(hc_packing *P, double *pos, double *quat, double *force, double *torque);
int hc_packing_pairs(int n, const double *size_a, const double *quat_a, const double *size_b, const double *quat_b, const double *rij,
                     const double *douter2, int rotate, double *lambda, double *f_ab_scl, double *nvec, double *f_a, double *t_a,
                     double *f_b, double *t_b, int *evals, int *kind);
int hc_packing_destroy(hc_packing *P);
/* Walls (this back end's own; the reference packs periodic boxes only).  hc_packing_set_walls, after hc_packing_create and
 * before the first hc_packing_run with max_steps > 0: mask is uint8 [dims0][dims1][dims2], 1 = wall, node i of an axis at
 * i * spacing grid cells; periodic[k] = 0 stops the wrap of positions and of pair separations on axis k.  A particle whose
 * centre lies at signed distance s < 0.55 Douter (its largest axis) from the wall surface gets one more partner, its own
 * mirror image across the tangent plane: same axes, centre x - 2 s n, orientation H R diag(1, 1, -1) with H = I - 2 n n^T.
 * s is the trilinear sample of the node field sqrt(d^2) - 1/2 (d: exact Euclidean distance in nodes to the nearest wall
 * node, truncated; -1/2 on wall nodes) times spacing minus wall_margin, n its normalised gradient (below 1e-12: no wall
 * partner that step).  The call builds the field on the device and repeats the first force evaluation.  Refused
 * (HC_ERR_ARG): a run has been made, walls are set already, fewer than 2 or more than 4096 nodes on an axis, a periodic
 * axis with dims * spacing != the box, a non-periodic one with (dims - 1) * spacing > the box or with a fluid node on one
 * of its two faces, a particle that starts on a wall node.  While walls are set, a centre that ends an iteration nearest
 * to a wall node, or off the mask on a non-periodic axis, sets the error flag to 2 (1 stays the root-search cap) and the
 * run returns HC_ERR_STATE.
 * hc_packing_wall_field: the node field [dims0][dims1][dims2], in node spacings.
 * hc_packing_walls probes the wall partner as hc_packing_pairs probes a pair: sizes [n][3], quaternions [n][4], s [n],
 * unit normals [n][3] into the fluid, douter2 [n].  Out: the particle's force and torque increments [n][3], the Dinner^2
 * candidate (douter2 unless the pair overlaps), the root search's evaluations and kind as in hc_packing_pairs.  The image
 * pair is evaluated at max(s, 1e-6); a torque whose direction is 0/0 (a principal axis along the normal) is returned as zero.
 * hc_packing_reserve_lists sets the partner lists' capacity per particle (at most N - 1; storage is never given back).  The
 * lists are rebuilt by every force evaluation, and one that does not fit grows them as status[11] describes, so a small
 * capacity costs one interrupted iteration; it is there to test that path. */
int hc_packing_set_walls(hc_packing *P, const unsigned char *mask, const int dims[3], double spacing, const int periodic[3],
                         double wall_margin);
int hc_packing_wall_field(hc_packing *P, double *s_node);
int hc_packing_reserve_lists(hc_packing *P, int capacity);
int hc_packing_walls(int n, const double *size, const double *quat, const double *s, const double *normal, const double *douter2,
                     int rotate, double *force, double *torque, double *candidate, int *evals, int *kind);

/* ------------------------------------------------------------------ running statistics
 * This back end's own.  The reference obtains time-averaged fields by writing whole fields to HDF5 every few thousand
 * iterations and averaging offline (io/FluidHdf5IO.hh, CellDensity :374-402); here the sums are kept on the device and a
 * sample is one or two kernels queued behind the step, with no host wait.
 * An hc_stats is bound to one lattice (n_slabs = 1; one handle per lattice) and, for the cell sets, to one container on
 * that lattice.  `what` is a mask of the sets; only those are allocated:
 *   HC_STATS_RHO_U         4 fp64 per node: what hcl_download_rho_u reports (1 + rhoBar; j / rho + (body + IBM force) / 2;
 *                          open-boundary nodes give the completed moments)
 *   HC_STATS_UU            6 fp64 per node: u_a u_b of that u (xx, xy, xz, yy, yz, zz), each product rounded, then added
 *   HC_STATS_PI            6 fp64 per node: what hcl_download_pi_neq reports
 *   HC_STATS_CELL_DENSITY  one 64-bit count per node and cell type: +1 per live vertex at its nearest node floor(p + 0.5),
 *                          wrapped on periodic axes and dropped outside the block on the others; removed particles and the
 *                          vertices of gone cells are not counted
 *   HC_STATS_INSIDE        one 64-bit count per node and cell type: +1 per COMPLETE cell of the type whose surface encloses
 *                          the node (the ray cast of the interior-viscosity pass: truncated bounding box, fluid nodes only,
 *                          odd parity; a cell whose box spans four periods tags nothing).  Two cells that overlap both
 *                          count, so a node's sum may exceed the number of samples.
 * The fluid sums are deterministic: one thread owns a node and samples are serial on the stream, so a sum equals the host
 * loop acc += value in sample order bit for bit.  The counts are integer atomics, hence order independent; being 64-bit they
 * cannot wrap and no sample cap applies.
 * hc_stats_set_every(S, every): hc_iterate samples after every iteration `it` with (it + 1) % every == 0, at the point where
 * the call would return had it ended there, so that a sample equals what hcl_download_rho_u, hcl_download_pi_neq, hcp_download
 * and hcp_download_alive would report then.  Such an iteration is not overlapped with the side stream.  every = 0 (the
 * default): explicit samples only.  hc_preinlet_iterate samples a lattice that carries a handle by the same rule at the end of
 * the coupled iteration, after the fluid hand-over and the cell check -- again where that call would return.  Cell types must
 * be added to the container before hc_stats_create with a cell set.
 * hc_stats_sample queues one sample now and does not wait.  hc_stats_reset zeroes the sums and the sample count.
 * hc_stats_download_fluid(S, set, out): the raw sums of ONE fluid set, [n][k] (k = 4: rho, u; 6; 6) in the reference node
 * order z + nz * (y + ny * x); hc_stats_download_cells(S, set, type, out): [n] counts of one cell set and type.  Both wait for
 * the queued work.  Divide by hc_stats_samples for means.
 * Refused (HC_ERR_ARG / HC_ERR_STATE, message in hc_last_error): a lattice with n_slabs > 1, a second hc_stats on a lattice,
 * a container bound to another lattice, a cell set without a container, an empty or unknown `what`, a negative cadence, a
 * type index out of range, a download of a set that was not selected (or of more than one set at once).
 * Lifetime: hcl_destroy and hcp_destroy REFUSE (HC_ERR_ARG) while an hc_stats refers to the lattice or the container; destroy
 * the hc_stats first.  The accumulators are not part of any checkpoint. */
#define HC_STATS_RHO_U 1
#define HC_STATS_UU 2
#define HC_STATS_PI 4
#define HC_STATS_CELL_DENSITY 8
#define HC_STATS_INSIDE 16
typedef struct hc_stats hc_stats;
int hc_stats_create(hc_lattice *L, hc_cells *C_or_null, int what, hc_stats **out);
int hc_stats_destroy(hc_stats *S);
int hc_stats_set_every(hc_stats *S, int every);
int hc_stats_sample(hc_stats *S);
int hc_stats_reset(hc_stats *S);
int hc_stats_samples(const hc_stats *S, long *n);
int hc_stats_download_fluid(hc_stats *S, int set, double *out);
int hc_stats_download_cells(hc_stats *S, int set, int type, long *out);

#ifdef __cplusplus
}
#endif
#endif
