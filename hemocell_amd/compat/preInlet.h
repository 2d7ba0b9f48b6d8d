// hemo::PreInlet (helper/preInlet.h of the reference): a periodic, driven copy of the inlet's cross-section that feeds the domain
// its inflow -- the fluid through Zou-He velocity nodes on the inlet plane, the cells by copying whole cells.
//
// The reference splits its MPI ranks into pre-inlet ranks and domain ranks; on the former hemocell.lattice IS the pre-inlet.
// This back end hands both over on the device between two lattices of ONE process (hcl_preinlet_*, hcp_preinlet_*,
// hc_preinlet_iterate), so the PreInlet object owns a second, hidden lattice and a second, hidden cell container:
// hemocell.lattice is always the domain, and hemocell.partOfpreInlet / preInlet->partOfpreInlet stay false.  What the
// reference's drivers do inside `if (hemocell.partOfpreInlet)` therefore never runs, and the facade does it for them
// (DESIGN.md section 6): the driving force after the first iteration, the pulsatile force once readNormalizedVelocities()
// has succeeded.  The geometry (location, fluidInlet, the send box and its offset) is a pure host function, preInletGeometry.
#pragma once
#include "hemocell.h"

enum Direction : int { Xpos, Xneg, Ypos, Yneg, Zpos, Zneg };   // helper/preInlet.h:42-44 (global, as in the reference)

#define DSET_SLICE 1000

namespace hemo {

inline plint cellsInBoundingBox(plb::Box3D const &box) { return std::abs((box.x1 - box.x0) * (box.y1 - box.y0) * (box.z1 - box.z0)); }

// ------------------------------------------------------------------ geometry (helper/preInlet.cpp:254-351, 399-422, 453-693)
struct PreInletGeometry {
  int axis = 0, sign = 0;           // X, Y, Z = 0, 1, 2; -1 for *neg (the pre-inlet lies below the domain), +1 for *pos
  plb::Box3D location;              // the pre-inlet's box, global coordinates
  plb::Box3D fluidInlet;            // the domain's inlet plane = the pre-inlet plane the velocities are read on
  plb::Box3D sendBox;               // particles on these nodes are sent (global coordinates, at the pre-inlet's far end)
  plb::Dot3D offset;                // added to a sent particle's position: +-lengthN on the axis
  string error;                     // empty, or the reference's refusal
};
inline plint &box_lo(plb::Box3D &b, int axis) { return axis == 0 ? b.x0 : axis == 1 ? b.y0 : b.z0; }
inline plint &box_hi(plb::Box3D &b, int axis) { return axis == 0 ? b.x1 : axis == 1 ? b.y1 : b.z1; }
inline plint box_lo(const plb::Box3D &b, int axis) { return axis == 0 ? b.x0 : axis == 1 ? b.y0 : b.z0; }
inline plint box_hi(const plb::Box3D &b, int axis) { return axis == 0 ? b.x1 : axis == 1 ? b.y1 : b.z1; }
inline void direction_axis(Direction d, int &axis, int &sign) {
  axis = (d == Xpos || d == Xneg) ? 0 : (d == Ypos || d == Yneg) ? 1 : 2;
  sign = (d == Xneg || d == Yneg || d == Zneg) ? -1 : 1;
}

// preInletFromSlice: the bounding box of the slice's fluid flags, enlarged by 1, extended by lengthN away from the domain and
// clipped to the lattice `system` on the two other axes (no lattice yet: no clip).  Then initializePreInletVelocityBoundary's
// fluidInlet, and applyPreInletParticleBoundary's send box and offset.
inline PreInletGeometry preInletGeometry(const plb::MultiScalarField3D<int> &flags, Direction direction, plb::Box3D boundary, plint lengthN,
                                         plint envelope, const plb::Box3D *system, const char *not_found = "(PreInlet) no preinlet found, is it in the correct location?") {
  PreInletGeometry g;
  direction_axis(direction, g.axis, g.sign);
  const int a = g.axis;
  if (box_lo(boundary, a) != box_hi(boundary, a)) { g.error = "Not a flat slice, refusing to create preInlet"; return g; }
  bool found = false; plb::Box3D bb;
  const plb::Box3D whole = flags.getBoundingBox();
  for (plint x = std::max(boundary.x0, whole.x0); x <= std::min(boundary.x1, whole.x1); x++)
    for (plint y = std::max(boundary.y0, whole.y0); y <= std::min(boundary.y1, whole.y1); y++)
      for (plint z = std::max(boundary.z0, whole.z0); z <= std::min(boundary.z1, whole.z1); z++) {
        if (!flags.get(x, y, z)) continue;
        if (!found) { bb = plb::Box3D(x, x, y, y, z, z); found = true; continue; }
        bb.x0 = std::min(bb.x0, x); bb.x1 = std::max(bb.x1, x); bb.y0 = std::min(bb.y0, y); bb.y1 = std::max(bb.y1, y); bb.z0 = std::min(bb.z0, z); bb.z1 = std::max(bb.z1, z);
      }
  if (!found) { g.error = not_found; return g; }
  g.location = plb::Box3D(bb.x0 - 1, bb.x1 + 1, bb.y0 - 1, bb.y1 + 1, bb.z0 - 1, bb.z1 + 1);
  if (g.sign < 0) box_lo(g.location, a) -= lengthN; else box_hi(g.location, a) += lengthN;
  if (system)
    for (int d = 0; d < 3; d++) {
      if (d == a) continue;
      box_lo(g.location, d) = std::max(box_lo(g.location, d), box_lo(*system, d));
      box_hi(g.location, d) = std::min(box_hi(g.location, d), box_hi(*system, d));
    }
  // :399-422: the flag matrix's box cut with location, flattened to its last plane (*neg) or its first (*pos)
  g.fluidInlet = plb::Box3D(std::max(whole.x0, g.location.x0), std::min(whole.x1, g.location.x1), std::max(whole.y0, g.location.y0),
                            std::min(whole.y1, g.location.y1), std::max(whole.z0, g.location.z0), std::min(whole.z1, g.location.z1));
  if (g.sign < 0) box_lo(g.fluidInlet, a) = box_hi(g.fluidInlet, a); else box_hi(g.fluidInlet, a) = box_lo(g.fluidInlet, a);
  // :267-335
  g.sendBox = g.fluidInlet;
  if (g.sign < 0) { box_lo(g.sendBox, a) = box_lo(g.fluidInlet, a) - lengthN; box_hi(g.sendBox, a) = box_lo(g.sendBox, a) + envelope; }
  else { box_hi(g.sendBox, a) = box_hi(g.fluidInlet, a) + lengthN; box_lo(g.sendBox, a) = box_hi(g.sendBox, a) - envelope; }
  const plint off = g.sign < 0 ? lengthN : -lengthN;
  g.offset = plb::Dot3D(a == 0 ? off : 0, a == 1 ? off : 0, a == 2 ? off : 0);
  return g;
}
// autoPreinletFromBoundary (:591-693): the slice is the plane one node inside the flag matrix's face on the direction's side
inline PreInletGeometry autoPreInletGeometry(const plb::MultiScalarField3D<int> &flags, Direction direction, plint lengthN, plint envelope, const plb::Box3D *system) {
  int a, sign; direction_axis(direction, a, sign);
  plb::Box3D slice = flags.getBoundingBox();
  if (sign < 0) { box_hi(slice, a) = box_lo(slice, a) + 1; box_lo(slice, a) = box_hi(slice, a); }
  else { box_lo(slice, a) = box_hi(slice, a) - 1; box_hi(slice, a) = box_lo(slice, a); }
  return preInletGeometry(flags, direction, slice, lengthN, envelope, system, "(PreInlet) no preinlet found, does fluid domain extend to the wall?");
}

// The cell hand-over's parameters (hcp_preinlet_create): the window along the axis in the pre-inlet's LOCAL coordinates, node 0
// at location's corner -- findParticles takes the particles whose nearest node lies in the send box, so its faces lie half a
// node outside -- and what an arriving cell's position is shifted by: local -> global, then the reference's offset
inline void preInletInjection(const PreInletGeometry &g, double window[2], double shift[3]) {
  const int a = g.axis;
  window[0] = (double)(box_lo(g.sendBox, a) - box_lo(g.location, a)) - 0.5;
  window[1] = (double)(box_hi(g.sendBox, a) - box_lo(g.location, a)) + 0.5;
  shift[0] = (double)(g.location.x0 + g.offset.x); shift[1] = (double)(g.location.y0 + g.offset.y); shift[2] = (double)(g.location.z0 + g.offset.z);
}

// PreInlet::interpolate (:841-870): piecewise linear in a table, clamped at the ends unless extrapolate
inline double preInletInterpolate(const vector<double> &xs, const vector<double> &ys, double x, bool extrapolate) {
  const size_t n = xs.size();
  size_t i = n - 2;                                      // the last interval, also for anything beyond it
  if (x < xs[n - 2]) { i = 0; while (x > xs[i + 1]) i++; }
  double y0 = ys[i], y1 = ys[i + 1];
  if (!extrapolate) {                                    // outside the table: the end value
    if (x < xs[i]) y1 = y0;
    if (x > xs[i + 1]) y0 = y1;
  }
  return y0 + (y1 - y0) / (xs[i + 1] - xs[i]) * (x - xs[i]);
}
// setDrivingForceTimeDependent (:874-886) without the direction: the factor the driving force is multiplied with at time t
inline double preInletPulseFactor(const vector<double> &times, const vector<double> &values, double average_vel, double pFrequency, double pulseEndTime, double t) {
  t *= pFrequency * pulseEndTime;
  t = std::fmod(t, pulseEndTime);
  return preInletInterpolate(times, values, t, false) / average_vel;
}

// boundaryFromFlagMatrix (helper/genericFunctions.cpp:138-159): walls around the flag matrix's box and on its 0 flags
inline void boundaryFromFlagMatrix(plb::MultiBlockLattice3D<T, DESCRIPTOR> *fluid, plb::MultiScalarField3D<int> *flagMatrix, bool partOfpreInlet) {
  const plb::Box3D d = flagMatrix->getBoundingBox();
  for (plint x = d.x0 - 1; x <= d.x1 + 1; x++) for (plint y = d.y0 - 1; y <= d.y1 + 1; y++) for (plint z = d.z0 - 1; z <= d.z1 + 1; z++)
    if ((x == d.x0 - 1 || y == d.y0 - 1 || z == d.z0 - 1 || x == d.x1 + 1 || y == d.y1 + 1 || z == d.z1 + 1) && !partOfpreInlet)
      defineDynamics(*fluid, x, y, z, new plb::BounceBack<T, DESCRIPTOR>(1.));
  for (plint x = d.x0; x <= d.x1; x++) for (plint y = d.y0; y <= d.y1; y++) for (plint z = d.z0; z <= d.z1; z++)
    if (flagMatrix->get(x, y, z) == 0 && !partOfpreInlet) defineDynamics(*fluid, x, y, z, new plb::BounceBack<T, DESCRIPTOR>(1.));
}

// ------------------------------------------------------------------ helper/preInlet.h:57-130
class PreInlet {
 public:
  PreInlet(HemoCell *hemocell_, plb::MultiScalarField3D<int> *flagMatrix_) : hemocell(hemocell_), flagMatrix(flagMatrix_) { read_length(); }
  // the management form: a flag matrix of ones with the lattice's walls as zeros (FillFlagMatrix, :728-740)
  PreInlet(HemoCell *hemocell_, plb::MultiBlockManagement3D &management) : hemocell(hemocell_) {
    flagMatrix = new plb::MultiScalarField3D<int>(management.nx, management.ny, management.nz, 1); owns_flags = true;
    auto *L = hemocell->lattice;
    for (plint x = 0; x < std::min(L->nx, flagMatrix->nx); x++) for (plint y = 0; y < std::min(L->ny, flagMatrix->ny); y++) for (plint z = 0; z < std::min(L->nz, flagMatrix->nz); z++)
      if (L->mask[((size_t)x * L->ny + y) * L->nz + z] != 0) flagMatrix->get(x, y, z) = 0;
    read_length();
  }
  ~PreInlet() {
    if (cells_handle) hcp_preinlet_destroy(cells_handle);
    if (fluid_handle) hcl_preinlet_destroy(fluid_handle);
    if (cells) hcp_destroy(cells);
    delete lattice;
    if (owns_flags) delete flagMatrix;
  }
  PreInlet(const PreInlet &) = delete;
  PreInlet &operator=(const PreInlet &) = delete;

  inline plint getNumberOfNodes() { return cellsInBoundingBox(location); }

  void preInletFromSlice(Direction direction_, plb::Box3D boundary) { take(direction_, &boundary); }
  void autoPreinletFromBoundary(Direction direction_) { take(direction_, nullptr); }

  // the domain's velocity nodes (one per fluid flag of the inlet plane, velocity zero) and the hidden lattice: location's
  // dimensions, periodic on the axis only, the inlet plane's flags extruded along it (createBoundary's rule, :940-986)
  void initializePreInletVelocityBoundary() {
    need_geometry("initializePreInlet");
    auto *bc = plb::createZouHeBoundaryCondition3D<T, DESCRIPTOR>();
    auto &D = *hemocell->lattice;
    const plb::Box3D f = fluidInlet;
    inlet_nodes.clear();
    for (plint x = f.x0; x <= f.x1; x++) for (plint y = f.y0; y <= f.y1; y++) for (plint z = f.z0; z <= f.z1; z++) {
      if (flagMatrix->get(x, y, z) != 1) continue;
      const plb::Box3D point(x, x, y, y, z, z);
      switch (direction) {
        case Xneg: bc->addVelocityBoundary0N(point, D); break;
        case Yneg: bc->addVelocityBoundary1N(point, D); break;
        case Zneg: bc->addVelocityBoundary2N(point, D); break;
        case Xpos: bc->addVelocityBoundary0P(point, D); break;
        case Ypos: bc->addVelocityBoundary1P(point, D); break;
        case Zpos: bc->addVelocityBoundary2P(point, D); break;
      }
      setBoundaryVelocity(D, point, plb::Array<T, 3>(0., 0., 0.));
      inlet_nodes.push_back({{x, y, z}});
    }
    delete bc;
    inlet_record = D.open_decls.size() - 1;
    inlet_first = inlet_nodes.empty() ? 0 : D.open_decls[inlet_record].values.size() - inlet_nodes.size();
    build_lattice();
  }
  void initializePreInletParticleBoundary() {}   // the send / receive maps of the reference's ranks: one process holds both sides here
  void initializePreInlet() { initializePreInletVelocityBoundary(); initializePreInletParticleBoundary(); }

  // On the domain the reference's loop changes nothing (its two wall tests lie outside the loop's range, and the rest is the
  // pre-inlet ranks'); the hidden lattice gets the pre-inlet ranks' part: wall wherever the inlet plane's flag is not fluid
  void createBoundary() {
    need_lattice("createBoundary");
    const int a = geometry.axis;
    const plb::Box3D whole = flagMatrix->getBoundingBox();
    lattice->bounce_back.assign(lattice->mask.size(), 0); lattice->bb_rho = 1.;
    for (plint x = location.x0; x <= location.x1; x++) for (plint y = location.y0; y <= location.y1; y++) for (plint z = location.z0; z <= location.z1; z++) {
      plint c[3] = {x, y, z}; c[a] = box_lo(fluidInlet, a);
      const bool inside = c[0] >= whole.x0 && c[0] <= whole.x1 && c[1] >= whole.y0 && c[1] <= whole.y1 && c[2] >= whole.z0 && c[2] <= whole.z1;
      const bool fluid = inside && flagMatrix->get(c[0], c[1], c[2]) != 0;
      const size_t k = ((size_t)(x - location.x0) * lattice->ny + (y - location.y0)) * lattice->nz + (z - location.z0);
      lattice->mask[k] = fluid ? 0 : 1; lattice->bounce_back[k] = fluid ? 0 : 1;   // BounceBack<T, DESCRIPTOR>(1.)
    }
    lattice->dirty_layout = true;
    lattice->periodicity().toggleAll(false); lattice->periodicity().toggle(a, true);
  }

  // :742-788: the fluid nodes of the pre-inlet's plane two inside its end, as the area of a circle
  void calculateDrivingForce() {
    need_lattice("calculateDrivingForce");
    const double re = (*hemocell->cfg)["preInlet"]["parameters"]["Re"].read<T>();
    const int a = geometry.axis;
    const plint n[3] = {lattice->nx, lattice->ny, lattice->nz};
    const plint plane = geometry.sign < 0 ? 2 : n[a] - 1 - 2;
    plint fluidArea = 0;
    for (plint x = 0; x < n[0]; x++) for (plint y = 0; y < n[1]; y++) for (plint z = 0; z < n[2]; z++) {
      const plint c[3] = {x, y, z};
      if (c[a] == plane && lattice->mask[((size_t)x * n[1] + y) * n[2] + z] == 0) fluidArea++;
    }
    T pipe_radius = std::sqrt(fluidArea / PI);
    hlog << "(Parameters) Your preInlet pipe has a calculated radius of " << pipe_radius << " LU, assuming a perfect circle" << std::endl;
    T u_lbm_max = re * param::nu_lbm / (pipe_radius * 2);
    drivingForce = 8 * param::nu_lbm * (u_lbm_max * 0.5) / pipe_radius / pipe_radius;
  }

  double average(vector<double> values) { double sum = 0.0; const int N = (int)values.size(); for (int i = 0; i < N; i++) sum += values[(size_t)i]; return sum / N; }
  double interpolate(vector<double> &xData, vector<double> &yData, double x, bool extrapolate) { return preInletInterpolate(xData, yData, x, extrapolate); }
  // :802-838.  From the moment it returns true the pre-inlet's force of iteration k is setDrivingForceTimeDependent(k * dt)
  bool readNormalizedVelocities() {
    std::string pulseFileName = (*hemocell->cfg)["preInlet"]["parameters"]["pulseFileName"].read<std::string>();
    std::ifstream pulseFile(pulseFileName);
    if (!pulseFile.is_open()) { cout << "*** WARNING! pulsatility data file " << pulseFileName << " does not exist!" << endl; return false; }
    for (std::string line; std::getline(pulseFile, line);) {   // "time value" per line
      std::istringstream fields(line); double t, v;
      if (fields >> t >> v) { normalizedVelocityTimes.push_back(t); normalizedVelocityValues.push_back(v); }
    }
    if (normalizedVelocityTimes.size() < 2) { cout << "*** WARNING! pulsatility data file " << pulseFileName << " holds fewer than two points!" << endl; return false; }
    average_vel = average(normalizedVelocityValues);
    pulseEndTime = normalizedVelocityTimes[normalizedVelocityTimes.size() - 1];
    try { pFrequency = (*hemocell->cfg)["preInlet"]["parameters"]["pFrequency"].read<double>(); }
    catch (const std::invalid_argument &) { pFrequency = 1.0 / pulseEndTime; }
    pulsatile = true;
    return true;
  }
  // The reference's drivers call these two on the pre-inlet's ranks only, where they write that lattice's force field.  Called
  // from a driver (which is the domain's side here) they write the hidden lattice's force for the iterations that follow; a
  // reference driver never gets here, and HemoCell::iterate() applies the same rule by itself (force_of_iteration)
  void setDrivingForce() { hemocell->flush(); explicit_force = true; explicit_value = drivingForce; }
  void setDrivingForceTimeDependent(double t) {
    hemocell->flush(); explicit_force = true;
    explicit_value = preInletPulseFactor(normalizedVelocityTimes, normalizedVelocityValues, average_vel, pFrequency, pulseEndTime, t) * drivingForce;
  }

  // applyPreInlet() after iterate() is one iteration of hc_preinlet_iterate(..., cells_every = 1); the pair is queued like
  // iterate() alone is.  Called on their own the two halves run at once
  void applyPreInletVelocityBoundary() { hemocell->flush(); ensure(); hc_check(hcl_preinlet_apply(fluid_handle), "hcl_preinlet_apply"); }
  void applyPreInletParticleBoundary() {
    hemocell->flush(); ensure();
    if (cells_handle) { hc_check(hcp_preinlet_apply(cells_handle, nullptr, nullptr), "hcp_preinlet_apply"); hemocell->cellfields->particleField.invalidate(); }
  }
  void applyPreInlet() {
    if (hemocell->pending > hemocell->pending_applied) { hemocell->pending_applied = hemocell->pending; return; }
    applyPreInletVelocityBoundary(); applyPreInletParticleBoundary();
  }
  // this back end's extension: {cells injected, rejected, removed by the sink, checks} (hcp_preinlet_counts)
  void cellCounts(long out[4]) {
    hemocell->flush();
    for (int i = 0; i < 4; i++) out[i] = 0;
    if (cells_handle) hc_check(hcp_preinlet_counts(cells_handle, out), "hcp_preinlet_counts");
  }

  Direction direction = Direction::Zneg;
  plb::Box3D location;
  plb::Box3D fluidInlet;
  int nProcs = 0;
  bool initialized = false;
  double drivingForce = 0.0;
  double average_vel = 0.0;
  double pulseEndTime = 1.0;
  double pFrequency = 1.0;
  std::vector<double> normalizedVelocityTimes;
  std::vector<double> normalizedVelocityValues;
  std::map<plint, plint> BlockToMpi;
  std::map<int, plint> particleSendMpi;
  std::map<int, bool> particleReceiveMpi;
  std::vector<plint> communicating_blocks;
  std::map<int, plb::Box3D> domain_at_rank;
  std::vector<int> my_send_blocks;
  std::vector<int> my_recv_blocks;
  int sendingBlocks = 0;
  bool partOfpreInlet = false;   // stays false: one process holds both lattices
  int inflow_length = 0;
  int preinlet_length = 0;
  bool communications_mapped = false;
  std::vector<int> particle_receivers;
  std::vector<int> particle_senders;
  HemoCell *hemocell;
  plb::MultiScalarField3D<int> *flagMatrix = 0;

  // ---- this back end's side
  PreInletGeometry geometry;
  plb::MultiBlockLattice3D<T, DESCRIPTOR> *lattice = nullptr;   // the hidden pre-inlet lattice, local coordinates = global - location's corner
  hc_cells *cells = nullptr;                                     // the hidden container
  hc_preinlet *fluid_handle = nullptr;
  hc_preinlet_cells *cells_handle = nullptr;
  bool owns_flags = false, pulsatile = false, explicit_force = false, particles_loaded = false, repulsion_pushed = false, boundary_repulsion_pushed = false;
  double explicit_value = 0.0;
  unsigned long iterations_begun = 0;
  std::array<T, 3> queued_force{{0, 0, 0}};
  std::vector<std::array<plint, 3>> inlet_nodes;
  size_t inlet_record = 0, inlet_first = 0;

  // the force the pre-inlet steps with in the iteration that starts at `iter`: none in the first iteration of the run (the
  // reference's drivers call setDrivingForce only after it), then drivingForce, or the pulse's value at iter * dt
  std::array<T, 3> force_of_iteration(unsigned int iter) const {
    double f = 0.0;
    if (explicit_force) f = explicit_value;
    else if (iterations_begun > 0) f = pulsatile ? preInletPulseFactor(normalizedVelocityTimes, normalizedVelocityValues, average_vel, pFrequency, pulseEndTime, iter * param::dt) * drivingForce : drivingForce;
    std::array<T, 3> F{{0, 0, 0}};
    F[(size_t)geometry.axis] = geometry.sign < 0 ? f : -f;
    return F;
  }
  void injection(double window[2], double shift[3]) const { preInletInjection(geometry, window, shift); }
  hc_cells *ensure_cells() {
    need_lattice("loadParticles");
    if (!cells) {
      hc_check(hcp_create(&cells, lattice->device_now(), &Parameters::raw()), "hcp_create");
      lattice->cells_bound = true;
      for (auto *f : hemocell->cellfields->cellFields) hc_check(hcp_add_type(cells, f->dev, (int)f->timescale, nullptr), "hcp_add_type");
    }
    HemoCell &h = *hemocell;
    if (h.boundaryRepulsionEnabled && !boundary_repulsion_pushed) { hc_check(hcp_set_boundary_repulsion(cells, h.boundaryRepulsionConstant_, h.boundaryRepulsionCutoff_, (int)h.boundaryRepulsionTimescale), "hcp_set_boundary_repulsion"); boundary_repulsion_pushed = true; }
    if (h.repulsionEnabled && !repulsion_pushed) { hc_check(hcp_set_repulsion(cells, h.repulsionConstant_, h.repulsionCutoff_, (int)h.repulsionTimescale), "hcp_set_repulsion"); repulsion_pushed = true; }
    return cells;
  }
  // everything the hand-over needs on the device: both lattices, both containers, the fluid coupling and -- once particles
  // were loaded and there are cell types -- the cell coupling with the sink on the domain face opposite the inlet
  void ensure() {
    need_lattice("applyPreInlet");
    HemoCell &h = *hemocell;
    hc_lattice *P = lattice->device_now();
    hc_lattice *D = h.lattice->device_now();
    hc_cells *dc = h.cellfields->device();
    ensure_cells();
    const int a = geometry.axis;
    if (!fluid_handle) {
      const plint n[3] = {lattice->nx, lattice->ny, lattice->nz};
      std::vector<int> idx;
      for (const auto &g : inlet_nodes) {
        const plint l[3] = {g[0] - location.x0, g[1] - location.y0, g[2] - location.z0};
        idx.push_back((int)(a == 0 ? l[1] * n[2] + l[2] : a == 1 ? l[0] * n[2] + l[2] : l[0] * n[1] + l[1]));
      }
      const int first = h.lattice->open_decls[inlet_record].first_slot + (int)inlet_first;
      hc_check(hcl_preinlet_create(&fluid_handle, P, D, a, (int)(box_lo(fluidInlet, a) - box_lo(location, a)), idx.data(), (int)idx.size(), first), "hcl_preinlet_create");
    }
    if (!cells_handle && particles_loaded && h.cellfields->size() > 0) {
      double window[2], shift[3]; injection(window, shift);
      const long stride = std::max<long>(1, h.cellfields->number_of_cells);   // the reference's number_of_cells
      hc_check(hcp_preinlet_create(&cells_handle, cells, dc, a, geometry.sign, window[0], window[1], shift, stride), "hcp_preinlet_create");
      const plint dn[3] = {h.lattice->nx, h.lattice->ny, h.lattice->nz};
      hc_check(hcp_preinlet_set_sink(cells_handle, 1, geometry.sign < 0 ? (double)(dn[a] - 1) : 0.0), "hcp_preinlet_set_sink");
    }
  }

 private:
  void read_length() { preinlet_length = (*hemocell->cfg)["preInlet"]["parameters"]["lengthN"].read<int>(); }
  void take(Direction direction_, const plb::Box3D *boundary) {
    if (global.world > 1) {
      hlog << "(PreInlet) (GPU backend) the pre-inlet runs beside the domain in one process; a run of " << global.world << " ranks is not part of this back end (DESIGN.md section 6), exiting ..." << endl;
      std::exit(1);
    }
    direction = direction_; initialized = true;
    inflow_length = (*hemocell->cfg)["domain"]["particleEnvelope"].read<int>();
    plb::Box3D system; const plb::Box3D *sys = nullptr;
    if (hemocell->lattice) { system = hemocell->lattice->getBoundingBox(); sys = &system; }
    geometry = boundary ? preInletGeometry(*flagMatrix, direction, *boundary, preinlet_length, inflow_length, sys)
                        : autoPreInletGeometry(*flagMatrix, direction, preinlet_length, inflow_length, sys);
    if (!geometry.error.empty()) { hlog << geometry.error << endl; std::exit(1); }
    if (!sys) hlog << (boundary ? "(PreInlet::preInletFromSlice) preInletFromSlice" : "(PreInlet::autoPreinletFromBoundary) autoPreinletFromBoundary") << " called without setting up a lattice first" << endl;
    location = geometry.location; fluidInlet = geometry.fluidInlet;
  }
  void need_geometry(const char *who) {
    if (!initialized) { hlog << "(PreInlet) " << who << " called before preInletFromSlice / autoPreinletFromBoundary" << endl; std::exit(1); }
    if (!hemocell->lattice) { hlog << "(PreInlet) " << who << " called without setting up a lattice first" << endl; std::exit(1); }
  }
  void need_lattice(const char *who) {
    if (!lattice) { hlog << "(PreInlet) " << who << " called before initializePreInlet" << endl; std::exit(1); }
  }
  void build_lattice() {
    delete lattice;
    plb::MultiBlockManagement3D m; m.nx = location.getNx(); m.ny = location.getNy(); m.nz = location.getNz();
    lattice = new plb::MultiBlockLattice3D<T, DESCRIPTOR>(m, nullptr, nullptr, nullptr, new plb::GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
    lattice->eq_rho = hemocell->lattice->eq_rho; for (int d = 0; d < 3; d++) lattice->eq_u[d] = hemocell->lattice->eq_u[d];
    createBoundary();
  }
};

// ------------------------------------------------------------------ HemoCell's side of the pre-inlet
inline HemoCell::~HemoCell() {
  flush(); hc_synchronize();
  delete preInlet;   // its couplings hold pointers into both lattices and containers
  delete cellfields; delete lattice; delete cfg; hc_comm_finalize(); global.hemoCellInitialized = false;
}
inline void HemoCell::preinlet_equilibrium(T rho, hemo::Array<T, 3> vel) {
  if (!preInlet->lattice) return;   // built later: it copies the domain's values then
  preInlet->lattice->eq_rho = rho; for (int d = 0; d < 3; d++) preInlet->lattice->eq_u[d] = vel[d];
  preInlet->lattice->dirty_layout = true;
}
// called by iterate() before it queues the iteration: the queue holds iterations that were followed by applyPreInlet() and all
// step the pre-inlet with one force
inline void HemoCell::preinlet_before_iterate() {
  PreInlet &p = *preInlet;
  if (pending > pending_applied) flush();
  const std::array<T, 3> F = p.force_of_iteration(iter);
  if (pending && F != p.queued_force) flush();
  p.queued_force = F;
  p.iterations_begun++;
}
inline void HemoCell::preinlet_run(long it, int n) {
  PreInlet &p = *preInlet;
  const int n_applied = std::min<int>((int)pending_applied, n);
  pending_applied = 0;
  p.ensure();
  if (!(p.lattice->active.base == p.queued_force)) { p.lattice->active.base = p.queued_force; p.lattice->dirty_force = true; }
  hc_lattice *P = p.lattice->device_now(), *D = lattice->device_now();
  const int ts = (int)queued_timescale;
  int done = 0;
  if (p.cells_handle && n_applied) { hc_check(hc_preinlet_iterate(p.fluid_handle, p.cells_handle, &it, n_applied, ts, 1, 1, /*cells_every=*/1), "hc_preinlet_iterate"); done = n_applied; }
  for (int s = done; s < n; s++) {   // no cell coupling (yet), or the last iteration, which applyPreInlet() has not followed
    long a = it;
    hc_check(hc_iterate(P, p.cells, &a, 1, ts, 1, 1), "iterate (pre-inlet)");
    hc_check(hc_iterate(D, cellfields->dev, &it, 1, ts, 1, 1), "iterate");
    if (s < n_applied) hc_check(hcl_preinlet_apply(p.fluid_handle), "hcl_preinlet_apply");
  }
  p.lattice->mark_stepped();
}
inline int HemoCell::preinlet_place(int type, int id, const double *p_lu, const double *angles, double min_dist_um) {
  PreInlet &p = *preInlet;
  if (!p.lattice) return 0;
  const plb::Box3D &b = p.location;
  const double lo[3] = {(double)b.x0, (double)b.y0, (double)b.z0}, hi[3] = {(double)b.x1, (double)b.y1, (double)b.z1};
  double local[3];
  for (int d = 0; d < 3; d++) { if (!(p_lu[d] > lo[d] - 0.5 && p_lu[d] <= hi[d] + 0.5)) return 0; local[d] = p_lu[d] - lo[d]; }
  int placed = 0;
  hc_check(hcp_add_cell(p.ensure_cells(), type, id, local, angles, min_dist_um, &placed), "hcp_add_cell");
  return placed;
}
inline void HemoCell::preinlet_loaded() {
  PreInlet &p = *preInlet;
  if (!p.lattice) return;
  hc_check(hcp_mechanics(p.ensure_cells(), (long)iter, 1), "hcp_mechanics");
  p.particles_loaded = true;
}
inline hc_cells *HemoCell::preinlet_cells() { return preInlet ? preInlet->cells : nullptr; }
inline const plb::Box3D *HemoCell::preinlet_box() { return preInlet ? &preInlet->location : nullptr; }

}  // namespace hemo

#include "hdf5_output.h"
namespace hemo {
inline bool HemoCell::preinlet_output_block(OutputBlock &blk) {
#ifdef HEMOCELL_WITH_HDF5
  if (!preInlet || !preInlet->lattice) return false;
  flush();
  blk.lattice = preInlet->lattice; blk.lattice->device_now();
  blk.cells = preInlet->cells; blk.id = global.world;
  blk.origin[0] = preInlet->location.x0; blk.origin[1] = preInlet->location.y0; blk.origin[2] = preInlet->location.z0;
  return true;
#else
  (void)blk; return false;
#endif
}
}  // namespace hemo

// what the reference's hemocell.h gives every case file next to this header (hemocell.h:46-53): the voxelizer and both namespaces
// opened -- cases/injured_vessel names HemoCell, Box3D and cout with no using-directive of its own
#include "helper/voxelizeDomain.h"
using namespace hemo;
using namespace plb;
