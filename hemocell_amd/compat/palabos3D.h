// Minimal stand-in for the Palabos names that HemoCell case drivers use on the hot path
// (SURVEY.md §8b "Palabos names the in-scope drivers also call").  This is NOT Palabos: the lattice
// object only records what the driver asked for (size, dynamics, bounce-back flags, periodicity, body
// force) and forwards the work to libhemocell_amd.so through the C ABI.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

extern "C" {
#include "hemocell_amd.h"
}

#ifndef HEMOCELL_T_DEFINED
#define HEMOCELL_T_DEFINED
typedef double T;                 // config/constant_defaults.h:117-119
#endif
typedef long int plint;           // config/constant_defaults.h:126-131
typedef long unsigned int pluint;

namespace plb {

using ::plint;
using ::pluint;

inline void hc_check(int rc, const char *what) {
  if (rc != 0) {   // the reference logs and exits (core/hemoCell.cpp:75-78)
    std::cerr << "(HemoCell) (GPU backend) " << what << ": " << hc_last_error() << std::endl;
    std::exit(1);
  }
}

template <typename U, int N>
struct Array {
  U data[N];
  Array() { for (int i = 0; i < N; i++) data[i] = U(); }
  Array(U a, U b) { static_assert(N == 2, "2 components"); data[0] = a; data[1] = b; }
  Array(U a, U b, U c) { static_assert(N == 3, "3 components"); data[0] = a; data[1] = b; data[2] = c; }
  U &operator[](int i) { return data[i]; }
  const U &operator[](int i) const { return data[i]; }
};

struct Dot3D { plint x, y, z; Dot3D(plint x_ = 0, plint y_ = 0, plint z_ = 0) : x(x_), y(y_), z(z_) {} };

struct Box3D {
  plint x0, x1, y0, y1, z0, z1;
  Box3D(plint a = 0, plint b = 0, plint c = 0, plint d = 0, plint e = 0, plint f = 0) : x0(a), x1(b), y0(c), y1(d), z0(e), z1(f) {}
  plint getNx() const { return x1 - x0 + 1; }
  plint getNy() const { return y1 - y0 + 1; }
  plint getNz() const { return z1 - z0 + 1; }
};

namespace descriptors {
template <typename U>
struct ForcedD3Q19Descriptor {
  enum { d = 3, q = 19 };
  struct ExternalField { enum { forceBeginsAt = 0, sizeOfForce = 3, numScalars = 3 }; };
};
}  // namespace descriptors

// ---- dynamics objects: only their identity and omega matter
template <typename U, template <typename> class D>
struct Dynamics {
  virtual ~Dynamics() {}
  virtual bool isBoundary() const { return false; }
  virtual U getOmega() const { return U(1); }
  virtual U wallDensity() const { return U(1); }
  virtual Dynamics *clone() const { return new Dynamics(*this); }
};
template <typename U, template <typename> class D>
struct GuoExternalForceBGKdynamics : Dynamics<U, D> {
  U omega;
  explicit GuoExternalForceBGKdynamics(U omega_) : omega(omega_) {}
  U getOmega() const override { return omega; }
  Dynamics<U, D> *clone() const override { return new GuoExternalForceBGKdynamics(*this); }
};
template <typename U, template <typename> class D>
struct BounceBack : Dynamics<U, D> {
  U rho;   // what computeDensity() answers on such a node (Palabos BounceBack); computeVelocity() answers zero
  explicit BounceBack(U rho_ = U(1)) : rho(rho_) {}
  bool isBoundary() const override { return true; }
  U wallDensity() const override { return rho; }
  Dynamics<U, D> *clone() const override { return new BounceBack(*this); }
};

struct MultiBlockManagement3D { plint nx = 0, ny = 0, nz = 0, envelope = 1; };

// names that only appear in signatures of the plugin surface (mechanics/cellMechanics.h:45, core/hemoCellField.h:67)
template <typename U, template <typename> class D>
struct BlockLattice3D { plint nx = 0, ny = 0, nz = 0; plint getNx() const { return nx; } plint getNy() const { return ny; } plint getNz() const { return nz; } };
template <typename U>
struct MeshMetrics {   // offLattice/triangularSurfaceMesh metrics the models read (mechanics/cellMechanics.h:50-78)
  U volume = 0, surface = 0, meanLength = 0; plint numVertices = 0, numTriangles = 0;
  U getVolume() const { return volume; } U getSurface() const { return surface; } U getMeanLength() const { return meanLength; }
  plint getNumVertices() const { return numVertices; } plint getNumTriangles() const { return numTriangles; }
};
struct BlockCommunicator3D {};
struct CombinedStatistics {};
template <typename U, template <typename> class D> struct MultiCellAccess3D {};

struct DefaultMultiBlockPolicy3D {
  MultiBlockManagement3D getMultiBlockManagement(plint nx, plint ny, plint nz, plint env = 1) const { MultiBlockManagement3D m; m.nx = nx; m.ny = ny; m.nz = nz; m.envelope = env; return m; }
  BlockCommunicator3D *getBlockCommunicator() const { return nullptr; }
  CombinedStatistics *getCombinedStatistics() const { return nullptr; }
  template <typename U, template <typename> class D> MultiCellAccess3D<U, D> *getMultiCellAccess() const { return nullptr; }
};
inline DefaultMultiBlockPolicy3D defaultMultiBlockPolicy3D() { return DefaultMultiBlockPolicy3D(); }

template <typename U>
class MultiScalarField3D {
 public:
  MultiScalarField3D(plint nx_, plint ny_, plint nz_, U v = U()) : nx(nx_), ny(ny_), nz(nz_), data((size_t)nx_ * ny_ * nz_, v) {}
  U &get(plint x, plint y, plint z) { return data[((size_t)x * ny + y) * nz + z]; }
  const U &get(plint x, plint y, plint z) const { return data[((size_t)x * ny + y) * nz + z]; }
  Box3D getBoundingBox() const { return Box3D(0, nx - 1, 0, ny - 1, 0, nz - 1); }
  plint getNx() const { return nx; }
  plint getNy() const { return ny; }
  plint getNz() const { return nz; }
  plint nx, ny, nz;
  std::vector<U> data;
};

template <typename U>
class VoxelizedDomain3D {
 public:
  explicit VoxelizedDomain3D(const MultiBlockManagement3D &m) : management(m) {}
  const MultiBlockManagement3D &getMultiBlockManagement() const { return management; }
  MultiBlockManagement3D management;
};

struct Periodicity3D {
  bool p[3] = {false, false, false};
  bool *changed = nullptr;   // set when a toggle really changes something; reading never does
  void toggleAll(bool v) { for (int a = 0; a < 3; a++) toggle(a, v); }
  void toggle(int axis, bool v) { if (p[axis] != v) { p[axis] = v; if (changed) *changed = true; } }
  bool get(int axis) const { return p[axis]; }
};

// The driver-facing lattice: a recorder in front of hc_lattice.  The device object is created on first
// use because drivers keep changing the description (periodicity, flags) after lattice->initialize().
// What the setExternalVector calls on a lattice add up to: one force for the whole domain plus a few boxes with their own
// (cases/kolmogorovFlow/kolmogorovFlow.cpp:136-140).  The library evaluates it inside its kernels (hcl_set_body_force,
// hcl_set_body_force_regions); no per-node force field exists on the host.
template <typename U>
struct ExternalForce {
  struct Region { Box3D box; std::array<U, 3> f; };
  std::array<U, 3> base{{U(0), U(0), U(0)}};
  std::vector<Region> regions;
  static bool same_box(const Box3D &a, const Box3D &b) { return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 && a.z0 == b.z0 && a.z1 == b.z1; }
  bool operator==(const ExternalForce &o) const {
    if (base != o.base || regions.size() != o.regions.size()) return false;
    for (size_t k = 0; k < regions.size(); k++) if (!same_box(regions[k].box, o.regions[k].box) || regions[k].f != o.regions[k].f) return false;
    return true;
  }
  void set(const Box3D &box, const Box3D &whole, const std::array<U, 3> &F) {
    if (box.x0 <= whole.x0 && box.x1 >= whole.x1 && box.y0 <= whole.y0 && box.y1 >= whole.y1 && box.z0 <= whole.z0 && box.z1 >= whole.z1) { base = F; regions.clear(); return; }
    for (size_t k = 0; k < regions.size(); k++) if (same_box(regions[k].box, box)) { regions.erase(regions.begin() + (long)k); break; }   // written again: it now overrides the others
    if (regions.size() == HC_MAX_FORCE_REGIONS) {
      std::cerr << "(HemoCell) (GPU backend) setExternalVector: more than " << HC_MAX_FORCE_REGIONS << " sub-domains with their own force" << std::endl;
      std::exit(1);
    }
    regions.push_back({box, F});
  }
  std::array<U, 3> at(plint x, plint y, plint z) const {
    std::array<U, 3> f = base;
    for (const Region &r : regions) if (x >= r.box.x0 && x <= r.box.x1 && y >= r.box.y0 && y <= r.box.y1 && z >= r.box.z0 && z <= r.box.z1) f = r.f;
    return f;
  }
};

template <typename U, template <typename> class D>
class MultiBlockLattice3D {
 public:
  MultiBlockLattice3D(const MultiBlockManagement3D &m, BlockCommunicator3D *, CombinedStatistics *, MultiCellAccess3D<U, D> *, Dynamics<U, D> *background)
      : nx(m.nx), ny(m.ny), nz(m.nz), omega(background ? background->getOmega() : U(1)), mask((size_t)m.nx * m.ny * m.nz, 0), background_dynamics(omega) { delete background; per.changed = &dirty_layout; }
  const Dynamics<U, D> &getBackgroundDynamics() const { return background_dynamics; }
  ~MultiBlockLattice3D() { if (dev) hcl_destroy(dev); }
  Box3D getBoundingBox() const { return Box3D(0, nx - 1, 0, ny - 1, 0, nz - 1); }
  plint getNx() const { return nx; }
  plint getNy() const { return ny; }
  plint getNz() const { return nz; }
  void toggleInternalStatistics(bool) {}
  Periodicity3D &periodicity() { return per; }
  // Palabos' initialize() runs the integrated data processors once: with a Lees-Edwards boundary installed
  // (hemo::LeesEdwardsBC::initialize) that is one pass, applied when the device lattice is created, or at once if it exists
  void initialize() {
    if (!le.on) return;
    le.init_pass = true; le.init_D = *le.cur;
    if (dev && !dirty_layout) { device(); le_pass_now(); }
  }
  void collideAndStream() { device(); le_sync(); hc_check(hcl_collide_stream(dev, 1), "collideAndStream"); }

  // ---- Lees-Edwards boundary (helper/leesEdwardsBC.h): the pass runs inside the library after every stream
  struct LeesEdwards {
    bool on = false, init_pass = false;
    double v_top = 0, v_bottom = 0, d = 0, init_D = 0;
    double *cur = nullptr;   // LeesEdwardsBC::LEcurrentDisplacement, what the driver updates
  } le;
  void le_sync() { if (le.on) hc_check(hcl_set_lees_edwards_displacement(dev, *le.cur, le.d), "hcl_set_lees_edwards_displacement"); }
  void le_pass_now() {
    hc_check(hcl_set_lees_edwards_displacement(dev, le.init_D, le.d), "hcl_set_lees_edwards_displacement");
    hc_check(hcl_lees_edwards_apply(dev), "hcl_lees_edwards_apply");
  }

  // ---- used by the shims below and by hemo::HemoCell
  // The device lattice of THIS rank: the whole domain on one GPU, or -- when the run was started as several ranks
  // (hc_comm_init_env in the HemoCell constructor) -- the x-slab [x0, x0 + nxl) of it, with the planes split as evenly as the
  // reference's block distribution does along one axis.  The driver keeps describing the global lattice.
  hc_lattice *device() {
    if (before_access) before_access();   // iterations the facade has queued run first (hemo::HemoCell::flush)
    sync_force();
    return device_now();
  }
  // The external force as the reference's field would hold it now: HemoCell::iterate() ends by zeroing it
  // (core/hemoCell.cpp:369-371) and drivers write it again around every iteration.
  ExternalForce<U> external_now() const { return force_cleared ? ExternalForce<U>() : applied; }
  // make it the one the device steps with; iterations queued under the previous one run first
  void sync_force() {
    const ExternalForce<U> e = external_now();
    if (e == active) return;
    if (before_access) before_access();
    active = e; dirty_force = true;
  }
  hc_lattice *device_now() {
    if (dev && !dirty_layout) { if (dirty_force) push_force(); if (dirty_open) push_open(); return dev; }
    if (dev && (stepped || cells_bound)) {
      std::cerr << "(HemoCell) (GPU backend) the lattice layout (dynamics / periodicity) was changed after " << (stepped ? "the first time step" : "the particles were loaded") << std::endl;
      std::exit(1);
    }
    if (dev) { hcl_destroy(dev); dev = nullptr; }
    int pr[3] = {per.p[0], per.p[1], per.p[2]};
    int tr = 0;
    hc_comm_info(&rank, &world, &tr);
    if (world == 1) hc_check(hc_init(0), "hc_init");
    x0 = (plint)rank * nx / world; nxl = (plint)(rank + 1) * nx / world - x0;
    hc_check(hcl_create(&dev, (int)nxl, (int)ny, (int)nz, pr, omega, (int)x0, (int)nx, world), "hcl_create");
    dev_generation++;   // what was bound to the previous device lattice (the CEPAC field, hemo::CEPACField) went with it
    std::vector<uint8_t> padded((size_t)(nxl + 4) * ny * nz, 1);   // beyond a non-periodic end: wall
    for (plint x = -2; x < nxl + 2; x++) {
      plint sx = x0 + x;
      if (sx < 0 || sx >= nx) { if (per.p[0]) sx = ((sx % nx) + nx) % nx; else continue; }
      std::copy(mask.begin() + (size_t)sx * ny * nz, mask.begin() + (size_t)(sx + 1) * ny * nz, padded.begin() + (size_t)(x + 2) * ny * nz);
    }
    hc_check(hcl_set_mask(dev, padded.data()), "hcl_set_mask");
    for (size_t k = 0; k < wall_u.size(); k++) { double w[3] = {wall_u[k][0], wall_u[k][1], wall_u[k][2]}; hc_check(hcl_set_wall_velocity(dev, 3 + (int)k, w), "hcl_set_wall_velocity"); }
    double u[3] = {eq_u[0], eq_u[1], eq_u[2]};
    hc_check(hcl_init_equilibrium(dev, eq_rho, u), "hcl_init_equilibrium");
    if (le.on) {
      hc_check(hcl_set_lees_edwards(dev, le.v_top, le.v_bottom), "hcl_set_lees_edwards");
      if (le.init_pass) le_pass_now();
    }
    dirty_layout = false; dirty_force = true;
    push_force();
    for (OpenDecl &d : open_decls) { d.first_slot = -1; d.dirty_values = true; }
    dirty_open = !open_decls.empty();
    if (dirty_open) push_open();
    return dev;
  }

  // ---- Zou-He open boundaries (OnLatticeBoundaryCondition3D::addVelocityBoundary0N ... addPressureBoundary2P, setBoundaryVelocity
  // and setBoundaryDensity on such nodes): recorded here in global coordinates, replayed on the device lattice after hcl_create.
  // Consecutive declarations of one kind, axis and side share a record, so a plane declared node by node (PreInlet) gets
  // consecutive slots.  The library's rules surface as refusals: a node declared twice, and Lees-Edwards beside open boundaries.
  struct OpenDecl {
    int kind, axis, orientation;
    std::vector<int> nodes;                 // [n][3] global coordinates, in declaration order
    std::vector<std::array<U, 4>> values;   // [n] {u_x, u_y, u_z, rho} as the driver set them
    int first_slot = -1, n_local = 0; bool dirty_values = true;   // this rank's slots (valid once pushed)
  };
  std::vector<OpenDecl> open_decls;
  std::vector<int> open_index;   // per node: (record << 1 | 1) ... 0 = none; empty until the first declaration
  bool dirty_open = false;
  [[noreturn]] static void refuse_open(const std::string &what) {
    std::cerr << "(HemoCell) (GPU backend) " << what << std::endl;
    std::exit(1);
  }
  void declare_open(int kind, int axis, int orientation, const Box3D &b) {
    if (le.on) refuse_open("open boundaries on a lattice with a Lees-Edwards boundary: the two do not combine");
    if (before_access) before_access();
    if (open_index.empty()) open_index.assign(mask.size(), 0);
    if (open_decls.empty() || open_decls.back().kind != kind || open_decls.back().axis != axis || open_decls.back().orientation != orientation || open_decls.back().first_slot >= 0) {
      OpenDecl d; d.kind = kind; d.axis = axis; d.orientation = orientation; open_decls.push_back(d);
    }
    OpenDecl &d = open_decls.back();
    for (plint x = b.x0; x <= b.x1; x++) for (plint y = b.y0; y <= b.y1; y++) for (plint z = b.z0; z <= b.z1; z++) {
      if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) refuse_open("open boundary: node (" + std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(z) + ") lies outside the lattice");
      int &slot = open_index[((size_t)x * ny + y) * nz + z];
      if (slot) refuse_open("open boundary: node (" + std::to_string(x) + ", " + std::to_string(y) + ", " + std::to_string(z) + ") declared twice (it is an open-boundary node already)");
      slot = (int)open_decls.size();
      d.nodes.push_back((int)x); d.nodes.push_back((int)y); d.nodes.push_back((int)z);
      d.values.push_back(std::array<U, 4>{{U(0), U(0), U(0), U(1)}});
    }
    dirty_open = true;
  }
  // setBoundaryVelocity / setBoundaryDensity on the declared nodes of a box; returns how many it reached
  size_t set_open_values(const Box3D &b, int kind, const U *v) {
    if (open_index.empty()) return 0;
    size_t hit = 0;
    for (OpenDecl &d : open_decls) {
      if (d.kind != kind) continue;
      for (size_t i = 0; i < d.values.size(); i++) {
        const int *c = &d.nodes[3 * i];
        if (c[0] < b.x0 || c[0] > b.x1 || c[1] < b.y0 || c[1] > b.y1 || c[2] < b.z0 || c[2] > b.z1) continue;
        if (kind == HC_OB_VELOCITY) { d.values[i][0] = v[0]; d.values[i][1] = v[1]; d.values[i][2] = v[2]; } else d.values[i][3] = v[0];
        if (!hit && before_access) before_access();
        d.dirty_values = true; hit++;
      }
    }
    if (hit) dirty_open = true;
    return hit;
  }
  // declare what is new on the device lattice and hand over the values that changed: every rank its own rows, in local coordinates
  void push_open() {
    if (le.on) refuse_open("open boundaries on a lattice with a Lees-Edwards boundary: the two do not combine");
    for (OpenDecl &d : open_decls) {
      std::vector<int> local; std::vector<double> u, rho;
      for (size_t i = 0; i < d.values.size(); i++) {
        const int *c = &d.nodes[3 * i];
        if (c[0] < x0 || c[0] >= x0 + nxl) continue;
        local.push_back(c[0] - (int)x0); local.push_back(c[1]); local.push_back(c[2]);
        u.push_back(d.values[i][0]); u.push_back(d.values[i][1]); u.push_back(d.values[i][2]); rho.push_back(d.values[i][3]);
      }
      if (d.first_slot < 0) {
        hc_check(hcl_open_boundary_add_axis(dev, d.kind, d.axis, d.orientation, local.data(), (int)(local.size() / 3), &d.first_slot), "hcl_open_boundary_add_axis");
        d.n_local = (int)(local.size() / 3); d.dirty_values = true;
      }
      if (d.dirty_values && d.n_local) {
        if (d.kind == HC_OB_VELOCITY) hc_check(hcl_open_boundary_set_velocity(dev, d.first_slot, d.n_local, u.data(), 0), "hcl_open_boundary_set_velocity");
        else hc_check(hcl_open_boundary_set_density(dev, d.first_slot, d.n_local, rho.data(), 0), "hcl_open_boundary_set_density");
      }
      d.dirty_values = false;
    }
    dirty_open = false;
  }
  void push_force() {
    double f[3] = {active.base[0], active.base[1], active.base[2]};
    hc_check(hcl_set_body_force(dev, f), "hcl_set_body_force");
    int boxes[6 * HC_MAX_FORCE_REGIONS]; double rf[3 * HC_MAX_FORCE_REGIONS];
    for (size_t k = 0; k < active.regions.size(); k++) {
      const Box3D &b = active.regions[k].box;
      const plint v[6] = {b.x0, b.x1, b.y0, b.y1, b.z0, b.z1};
      for (int i = 0; i < 6; i++) boxes[6 * k + i] = (int)v[i];
      for (int d = 0; d < 3; d++) rf[3 * k + d] = active.regions[k].f[d];
    }
    hc_check(hcl_set_body_force_regions(dev, (int)active.regions.size(), boxes, rf), "hcl_set_body_force_regions");
    dirty_force = false;
  }
  void mark_stepped() { stepped = true; }

  // velocity-wall classes (mask values 3..6), helper/hemocellInit.hh:71-86
  int wall_class(U a, U b, U c) {
    for (size_t k = 0; k < wall_u.size(); k++) if (wall_u[k][0] == a && wall_u[k][1] == b && wall_u[k][2] == c) return 3 + (int)k;
    if (wall_u.size() == 4) { std::cerr << "(HemoCell) (GPU backend) at most four distinct wall velocities are supported" << std::endl; std::exit(1); }
    wall_u.push_back({a, b, c});
    return 3 + (int)wall_u.size() - 1;
  }
  std::vector<std::array<U, 3>> wall_u;
  void note_wall(size_t k, bool wall, const Dynamics<U, D> *dyn) {
    if (wall && bounce_back.empty()) bounce_back.assign(mask.size(), 0);
    if (!bounce_back.empty()) bounce_back[k] = wall ? 1 : 0;
    if (wall) bb_rho = dyn->wallDensity();
  }

  plint nx, ny, nz;
  U omega;
  std::vector<uint8_t> mask;   // 1 = BounceBack / isBoundary, 3..6 = velocity wall classes
  std::vector<uint8_t> bounce_back;   // 1 where a BounceBack dynamics was assigned (output: velocity 0, density bb_rho); empty = none
  U bb_rho = 1;
  Periodicity3D per;
  U eq_rho = 1; U eq_u[3] = {0, 0, 0};
  ExternalForce<U> applied, active;   // written by the driver since the field was last zeroed / what the device steps with
  bool force_cleared = false;         // an iterate() has zeroed the field and nothing was written since
  std::function<void()> before_access;
  bool dirty_layout = true, dirty_force = true, stepped = false, cells_bound = false;
  long dev_generation = 0;   // counts the device lattices created so far
  hc_lattice *dev = nullptr;
  int rank = 0, world = 1; plint x0 = 0, nxl = 0;   // this rank's slab (valid once device() ran)
  GuoExternalForceBGKdynamics<U, D> background_dynamics;   // what the lattice was constructed with (getBackgroundDynamics)
};

// defineDynamics(lattice, flagMatrix, bbox, new BounceBack(1.), flag)   (examples/pipeflow/pipeflow.cpp:73)
template <typename U, template <typename> class D>
void defineDynamics(MultiBlockLattice3D<U, D> &lattice, MultiScalarField3D<int> &flags, Box3D box, Dynamics<U, D> *dyn, int whichFlag) {
  const bool wall = dyn->isBoundary();
  for (plint x = box.x0; x <= box.x1; x++)
    for (plint y = box.y0; y <= box.y1; y++)
      for (plint z = box.z0; z <= box.z1; z++)
        if (flags.get(x, y, z) == whichFlag) { const size_t k = ((size_t)x * lattice.ny + y) * lattice.nz + z; lattice.mask[k] = wall ? 1 : 0; lattice.note_wall(k, wall, dyn); }
  if (lattice.before_access) lattice.before_access();
  lattice.dirty_layout = true;
  delete dyn;
}
// domain-functional form: the nodes of the box the driver's predicate picks (examples/flowaroundsphere/flowaroundsphere.cpp:38-57,
// cases/stenosis/stenosis.cpp:38-60)
struct DomainFunctional3D {
  virtual ~DomainFunctional3D() {}
  virtual bool operator()(plint iX, plint iY, plint iZ) const = 0;
  virtual DomainFunctional3D *clone() const = 0;
};
template <typename U, template <typename> class D>
void defineDynamics(MultiBlockLattice3D<U, D> &lattice, Box3D box, DomainFunctional3D *domain, Dynamics<U, D> *dyn) {
  const bool wall = dyn->isBoundary();
  for (plint x = std::max<plint>(box.x0, 0); x <= std::min<plint>(box.x1, lattice.nx - 1); x++)
    for (plint y = std::max<plint>(box.y0, 0); y <= std::min<plint>(box.y1, lattice.ny - 1); y++)
      for (plint z = std::max<plint>(box.z0, 0); z <= std::min<plint>(box.z1, lattice.nz - 1); z++)
        if ((*domain)(x, y, z)) { const size_t k = ((size_t)x * lattice.ny + y) * lattice.nz + z; lattice.mask[k] = wall ? 1 : 0; lattice.note_wall(k, wall, dyn); }
  lattice.dirty_layout = true;
  delete domain; delete dyn;
}
// box form (e.g. cases with explicit wall slabs)
template <typename U, template <typename> class D>
void defineDynamics(MultiBlockLattice3D<U, D> &lattice, Box3D box, Dynamics<U, D> *dyn) {
  const bool wall = dyn->isBoundary();
  for (plint x = box.x0; x <= box.x1; x++)
    for (plint y = box.y0; y <= box.y1; y++)
      for (plint z = box.z0; z <= box.z1; z++) { const size_t k = ((size_t)x * lattice.ny + y) * lattice.nz + z; lattice.mask[k] = wall ? 1 : 0; lattice.note_wall(k, wall, dyn); }
  lattice.dirty_layout = true;
  delete dyn;
}

// point form (helper/genericFunctions.cpp:138-159, helper/preInlet.cpp:940-986); a node outside the lattice is nobody's
template <typename U, template <typename> class D>
void defineDynamics(MultiBlockLattice3D<U, D> &lattice, plint x, plint y, plint z, Dynamics<U, D> *dyn) {
  if (x >= 0 && y >= 0 && z >= 0 && x < lattice.nx && y < lattice.ny && z < lattice.nz) {
    const bool wall = dyn->isBoundary();
    const size_t k = ((size_t)x * lattice.ny + y) * lattice.nz + z;
    lattice.mask[k] = wall ? 1 : 0; lattice.note_wall(k, wall, dyn); lattice.dirty_layout = true;
  }
  delete dyn;
}

// setExternalVector(lattice, bbox, forceBeginsAt, F)   (core/hemoCell.cpp:369-371, examples/pipeflow/pipeflow.cpp:144-146)
template <typename U, template <typename> class D>
void setExternalVector(MultiBlockLattice3D<U, D> &lattice, Box3D box, int, Array<U, 3> F) {
  if (lattice.force_cleared) { lattice.applied = ExternalForce<U>(); lattice.force_cleared = false; }
  lattice.applied.set(box, lattice.getBoundingBox(), std::array<U, 3>{{F[0], F[1], F[2]}});   // reaches the device at the next step or look (sync_force)
}

// ---- boundary-condition names of examples/stretchCell/stretchCell.cpp:74-79 and helper/hemocellInit.hh:71-86.
// A "velocity condition" node becomes a no-slip wall node moving with the velocity given by
// setBoundaryVelocity (full-way bounce-back + Ladd momentum term inside the library).  Palabos' regularised
// velocity nodes are isBoundary() as well, so the IBM treats both alike.
namespace boundary { enum BcType { dirichlet, neumann, freeslip, density, outflow, normalOutflow }; }   // boundaryCondition3D.h

template <typename U, template <typename> class D>
struct OnLatticeBoundaryCondition3D {
  virtual ~OnLatticeBoundaryCondition3D() {}
  // Zou-He nodes (boundaryCondition/boundaryCondition3D.h): <axis><N / P>; the library completes the unknown populations
  // inside its collide (hcl_open_boundary_add_axis).  Only the Zou-He conditions exist: a velocity is dirichlet, a pressure
  // dirichlet or density (the other BcType values are refused)
  void add_open(int kind, int axis, int orientation, Box3D b, MultiBlockLattice3D<U, D> &l, boundary::BcType t, const char *name) {
    if (t != boundary::dirichlet && !(kind == HC_OB_PRESSURE && t == boundary::density)) MultiBlockLattice3D<U, D>::refuse_open(std::string(name) + ": only boundary::dirichlet velocity and boundary::density pressure nodes are part of this back end");
    l.declare_open(kind, axis, orientation, b);
  }
#define HEMOCELL_OPEN_BOUNDARY(AXIS, SIDE, ORIENTATION) \
  void addVelocityBoundary##AXIS##SIDE(Box3D b, MultiBlockLattice3D<U, D> &l, boundary::BcType t = boundary::dirichlet) { add_open(HC_OB_VELOCITY, AXIS, ORIENTATION, b, l, t, "addVelocityBoundary" #AXIS #SIDE); } \
  void addPressureBoundary##AXIS##SIDE(Box3D b, MultiBlockLattice3D<U, D> &l, boundary::BcType t = boundary::dirichlet) { add_open(HC_OB_PRESSURE, AXIS, ORIENTATION, b, l, t, "addPressureBoundary" #AXIS #SIDE); }
  HEMOCELL_OPEN_BOUNDARY(0, N, -1) HEMOCELL_OPEN_BOUNDARY(0, P, 1)
  HEMOCELL_OPEN_BOUNDARY(1, N, -1) HEMOCELL_OPEN_BOUNDARY(1, P, 1)
  HEMOCELL_OPEN_BOUNDARY(2, N, -1) HEMOCELL_OPEN_BOUNDARY(2, P, 1)
#undef HEMOCELL_OPEN_BOUNDARY
  void setVelocityConditionOnBlockBoundaries(MultiBlockLattice3D<U, D> &l) {
    for (plint x = 0; x < l.nx; x++) for (plint y = 0; y < l.ny; y++) for (plint z = 0; z < l.nz; z++)
      if (x == 0 || y == 0 || z == 0 || x == l.nx - 1 || y == l.ny - 1 || z == l.nz - 1) l.mask[((size_t)x * l.ny + y) * l.nz + z] = 1;
    l.dirty_layout = true;
  }
  void setVelocityConditionOnBlockBoundaries(MultiBlockLattice3D<U, D> &l, Box3D b) {
    for (plint x = b.x0; x <= b.x1; x++) for (plint y = b.y0; y <= b.y1; y++) for (plint z = b.z0; z <= b.z1; z++) l.mask[((size_t)x * l.ny + y) * l.nz + z] = 1;
    l.dirty_layout = true;
  }
};
template <typename U, template <typename> class D>
OnLatticeBoundaryCondition3D<U, D> *createLocalBoundaryCondition3D() { return new OnLatticeBoundaryCondition3D<U, D>(); }
// boundaryCondition/boundaryInstantiator3D.h, zouHeBoundary3D.h: the names drivers build a Zou-He condition from
template <typename U, template <typename> class D> struct WrappedZouHeBoundaryManager3D {};
template <typename U, template <typename> class D, class Manager>
struct BoundaryConditionInstantiator3D : OnLatticeBoundaryCondition3D<U, D> {};
template <typename U, template <typename> class D>
OnLatticeBoundaryCondition3D<U, D> *createZouHeBoundaryCondition3D() { return new BoundaryConditionInstantiator3D<U, D, WrappedZouHeBoundaryManager3D<U, D>>(); }
template <typename U, template <typename> class D>
void setBoundaryVelocity(MultiBlockLattice3D<U, D> &l, Box3D b, Array<U, 3> v) {
  l.set_open_values(b, HC_OB_VELOCITY, &v[0]);   // declared open velocity nodes take it as their slot's velocity
  const bool still = (v[0] == 0 && v[1] == 0 && v[2] == 0);
  const int cls = still ? 1 : l.wall_class(v[0], v[1], v[2]);
  for (plint x = b.x0; x <= b.x1; x++) for (plint y = b.y0; y <= b.y1; y++) for (plint z = b.z0; z <= b.z1; z++) {
    uint8_t &m = l.mask[((size_t)x * l.ny + y) * l.nz + z];
    if (m != 0 && m != (uint8_t)cls) { m = (uint8_t)cls; l.dirty_layout = true; }   // only nodes that carry a velocity condition
  }
}
template <typename U, template <typename> class D>
void setBoundaryDensity(MultiBlockLattice3D<U, D> &l, Box3D b, U rho) { l.set_open_values(b, HC_OB_PRESSURE, &rho); }

template <typename U, template <typename> class D>
std::string getMultiBlockInfo(MultiBlockLattice3D<U, D> &l) {
  int rank = 0, world = 1, tr = 0; hc_comm_info(&rank, &world, &tr);
  // the reference's text names the atomic-block layout in this line, and its CI drops lines with "atomic-block" when it
  // compares the logs of runs with different rank counts (scripts/ci/pipeflow_sanity.sh:30)
  return "Size of the lattice: " + std::to_string(l.nx) + "-by-" + std::to_string(l.ny) + "-by-" + std::to_string(l.nz) + " in " + std::to_string(world) + " atomic-block(s): one x-slab per rank and GPU";
}

// plb::pcout: rank 0 only
struct Pcout {
  static bool main() { int r = 0; hc_comm_info(&r, nullptr, nullptr); return r == 0; }
  template <typename V> Pcout &operator<<(const V &v) { if (main()) std::cout << v; return *this; }
  Pcout &operator<<(std::ostream &(*f)(std::ostream &)) { if (main()) std::cout << f; return *this; }
};
static Pcout pcout;
typedef std::ofstream plb_ofstream;

}  // namespace plb
