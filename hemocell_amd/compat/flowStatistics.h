// Running flow and hematocrit statistics through the facade: hemo::FlowStatistics.  This back end's own (the reference averages
// its HDF5 output offline): the sums live on the device (hc_stats, csrc/stats.hip) and are sampled inside HemoCell::iterate()
// at a cadence, with no host wait; write() puts the means beside the fluid output.
//
//   FlowStatistics stats(hemocell);                       // after the HemoCell, so that it is destroyed before it
//   stats.enable(5, {OUTPUT_VELOCITY, OUTPUT_CELL_DENSITY});   // after loadParticles(): the cell types must exist
//   ... hemocell.iterate() ...
//   stats.write();      // <out>/hdf5/<iter>/Statistics.<iter>.p.<block>.h5
//
// enable(every, outputs) maps the existing output names to the sets:
//   OUTPUT_VELOCITY      -> MeanVelocity [3] and VelocityCovariance [6] = <u_a u_b> - <u_a><u_b> (xx, xy, xz, yy, yz, zz)
//   OUTPUT_DENSITY       -> MeanDensity [1]
//   OUTPUT_SHEAR_STRESS  -> MeanShearStress [6] = (omega / 2 - 1) <PiNeq> with the lattice's omega, zero on BounceBack nodes
//   OUTPUT_CELL_DENSITY  -> per cell type CellDensity_<name> [1] (mean vertices per node) and Hematocrit_<name> [1] (the fraction
//                           of the samples in which the node lay inside a cell of the type; fluid nodes only; two cells that
//                           overlap on a node both count)
// Any other name is skipped with one log line.  The file has the fluid file's layout (compat/hdf5_output.h): float32
// [Nz+2][Ny+2][Nx+2][C] with a one-node envelope (periodic image, or the face again where the domain ends), the same attributes
// and, with outputInSiUnits, the scaling of the instantaneous fields (velocity dx/dt, covariance its square, density and stress
// df/dx^2, CellDensity the type's volumeFractionOfLspPerNode).  Wall nodes answer as in the fluid file: a BounceBack node zero
// velocity and its density, a velocity wall its velocity.  CellDensity sits at the node itself, as every other dataset does
// (the instantaneous CellDensity keeps the reference's offset of one node).
// An iteration that is sampled is one the library does not overlap with its side stream.  The accumulators are not checkpointed:
// saveCheckPoint says so once, and loadCheckPoint leaves them reset.  Several ranks and a pre-inlet are refused.
#pragma once
#include "hemocell.h"

namespace hemo {

class FlowStatistics {
 public:
  explicit FlowStatistics(HemoCell &hemocell_) : h(hemocell_) {
    if (global.world > 1) h.refuse("FlowStatistics on several ranks (running statistics need the whole domain on one GPU)");
    if (h.flowStatisticsReset) { hlog << "(HemoCell) (FlowStatistics) only one FlowStatistics per HemoCell, exiting ..." << endl; std::exit(1); }
    h.flowStatisticsReset = [this] { if (S) reset(); };
  }
  ~FlowStatistics() { if (S) hc_stats_destroy(S); h.flowStatisticsReset = nullptr; }
  FlowStatistics(const FlowStatistics &) = delete;
  void operator=(const FlowStatistics &) = delete;

  void enable(unsigned int every, vector<int> outputs) {
    if (h.preInlet) h.refuse("FlowStatistics beside a pre-inlet");
    if (S) { hlog << "(HemoCell) (FlowStatistics) enable() was called twice, exiting ..." << endl; std::exit(1); }
    what = 0;
    for (int var : outputs) {
      if (var == OUTPUT_VELOCITY) what |= HC_STATS_RHO_U | HC_STATS_UU;
      else if (var == OUTPUT_DENSITY) what |= HC_STATS_RHO_U;
      else if (var == OUTPUT_SHEAR_STRESS) what |= HC_STATS_PI;
      else if (var == OUTPUT_CELL_DENSITY) what |= HC_STATS_CELL_DENSITY | HC_STATS_INSIDE;
      else { hlog << "(HemoCell) (FlowStatistics) output variable " << var << " has no running statistic and is skipped" << endl; continue; }
      variables.push_back(var);
    }
    if (!what) { hlog << "(HemoCell) (FlowStatistics) enable() names no statistic, exiting ..." << endl; std::exit(1); }
    // binding the container freezes the lattice's layout (palabos3D.h, device_now), so the handle never sees its lattice replaced
    hc_cells *c = h.cellfields->device();
    hc_check(hc_stats_create(h.lattice->device(), c, what, &S), "hc_stats_create");
    hc_check(hc_stats_set_every(S, (int)every), "hc_stats_set_every");
    hlog << "(HemoCell) (FlowStatistics) sampling every " << every << " iterations" << endl;
  }
  long samples() { long n = 0; hc_check(hc_stats_samples(device(), &n), "hc_stats_samples"); return n; }
  void reset() { hc_check(hc_stats_reset(device()), "hc_stats_reset"); }
  // the raw sums of one fluid set, [n][4] (HC_STATS_RHO_U) or [n][6], and the raw counts of one cell set and type, [n]; node
  // order z + nz * (y + ny * x)
  vector<double> sums(int set) {
    vector<double> out(nodes() * (size_t)(set == HC_STATS_RHO_U ? 4 : 6));
    hc_check(hc_stats_download_fluid(device(), set, out.data()), "hc_stats_download_fluid");
    return out;
  }
  vector<long> counts(int set, unsigned int type) {
    vector<long> out(nodes());
    hc_check(hc_stats_download_cells(device(), set, (int)type, out.data()), "hc_stats_download_cells");
    return out;
  }
  // queued iterations run first (lattice->device() flushes the facade's queue)
  hc_stats *device() {
    if (!S) { hlog << "(HemoCell) (FlowStatistics) enable() has not been called, exiting ..." << endl; std::exit(1); }
    h.lattice->device();
    return S;
  }
  inline void write();

 private:
  size_t nodes() const { return (size_t)h.lattice->nx * h.lattice->ny * h.lattice->nz; }
  HemoCell &h;
  hc_stats *S = nullptr;
  int what = 0;
  vector<int> variables;
};

inline void FlowStatistics::write() {
  if (h.preInlet) h.refuse("FlowStatistics beside a pre-inlet");
  const long ns = samples();
#ifdef HEMOCELL_WITH_HDF5
  if (ns == 0) { hlog << "(HemoCell) (FlowStatistics) no samples yet: nothing is written at " << h.iter << endl; return; }
  auto *L = h.lattice;
  const plint nx = L->nx, ny = L->ny, nz = L->nz;
  const string dir = h.outDir + "/hdf5/" + zeroPadNumber(h.iter);
  mkdir((h.outDir + "/hdf5").c_str(), 0755); mkdir(dir.c_str(), 0755);
  const string fileName = dir + "/Statistics." + zeroPadNumber(h.iter) + ".p." + std::to_string(global.rank) + ".h5";
  hlog << "(HemoCell) (FlowStatistics) writing the means of " << ns << " samples at timestep " << h.iter << endl;
  hid_t file = H5Fcreate(fileName.c_str(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT);
  double dx = Parameters::dx, dt = Parameters::dt; long it = h.iter, nsamp = ns; int id = global.rank;
  H5LTset_attribute_double(file, "/", "dx", &dx, 1); H5LTset_attribute_double(file, "/", "dt", &dt, 1);
  H5LTset_attribute_long(file, "/", "iteration", &it, 1); H5LTset_attribute_int(file, "/", "processorId", &id, 1);
  H5LTset_attribute_long(file, "/", "numberOfSamples", &nsamp, 1);
  const hsize_t Nx = nx + 2, Ny = ny + 2, Nz = nz + 2;
  int ncells = (int)(Nx * Ny * Nz); int sub[3] = {(int)Nz, (int)Ny, (int)Nx};
  float dxdydz[3] = {1.f, 1.f, 1.f}, rel[3] = {-1.5f, -1.5f, -1.5f};
  const bool si = h.outputInSiUnits;
  if (si) for (int k = 0; k < 3; k++) { rel[k] *= (float)Parameters::dx; dxdydz[k] = (float)Parameters::dx; }
  H5LTset_attribute_int(file, "/", "numberOfCells", &ncells, 1); H5LTset_attribute_int(file, "/", "subdomainSize", sub, 3);
  H5LTset_attribute_float(file, "/", "relativePosition", rel, 3); H5LTset_attribute_float(file, "/", "dxdydz", dxdydz, 3);
  // node of the lattice behind output node (x, y, z) in -1 .. n: the periodic image, or the face again where the domain ends
  auto src = [](plint v, plint n, bool per) { if (v < 0 || v >= n) return per ? ((v % n) + n) % n : std::min<plint>(std::max<plint>(v, 0), n - 1); return v; };
  auto write4 = [&](const string &name, int C, const std::function<double(size_t, int)> &val) {   // val(node, component)
    vector<float> out((size_t)(Nx * Ny * Nz) * C); size_t o = 0;
    for (plint z = -1; z <= nz; z++) for (plint y = -1; y <= ny; y++) for (plint x = -1; x <= nx; x++) {
      const size_t k = ((size_t)src(x, nx, L->per.p[0]) * ny + (size_t)src(y, ny, L->per.p[1])) * nz + (size_t)src(z, nz, L->per.p[2]);
      for (int c = 0; c < C; c++) out[o++] = (float)val(k, c);
    }
    hsize_t dim[4] = {Nz, Ny, Nx, (hsize_t)C}, chunk[4] = {std::min<hsize_t>(1000, Nz), std::min<hsize_t>(1000, Ny), std::min<hsize_t>(1000, Nx), (hsize_t)C};
    hid_t sid = H5Screate_simple(4, dim, NULL), pl = H5Pcreate(H5P_DATASET_CREATE);
    H5Pset_chunk(pl, 4, chunk); H5Pset_deflate(pl, 7);
    hid_t did = H5Dcreate2(file, name.c_str(), H5T_NATIVE_FLOAT, sid, H5P_DEFAULT, pl, H5P_DEFAULT);
    H5Dwrite(did, H5T_NATIVE_FLOAT, H5S_ALL, H5S_ALL, H5P_DEFAULT, out.data());
    H5Dclose(did); H5Pclose(pl); H5Sclose(sid);
  };
  const double n = (double)ns;
  const double s_u = si ? Parameters::dx / Parameters::dt : 1.0, s_stress = si ? Parameters::df / (Parameters::dx * Parameters::dx) : 1.0;
  // what the node's dynamics answer on a wall, as in the fluid file
  auto is_bb = [&](size_t k) { return !L->bounce_back.empty() && L->bounce_back[k]; };
  auto wall_velocity = [&](size_t k, int c) { const uint8_t m = L->mask[k]; return m >= 3 && !is_bb(k) ? (double)L->wall_u[(size_t)(m - 3)][(size_t)c] : 0.0; };
  vector<double> ru, uu, pi;
  if (what & HC_STATS_RHO_U) ru = sums(HC_STATS_RHO_U);
  for (int var : variables) {
    if (var == OUTPUT_VELOCITY) {
      uu = sums(HC_STATS_UU);
      write4("MeanVelocity", 3, [&](size_t k, int c) { return (L->mask[k] ? wall_velocity(k, c) : ru[4 * k + 1 + c] / n) * s_u; });
      static const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
      write4("VelocityCovariance", 6, [&](size_t k, int c) {
        if (L->mask[k]) return 0.0;
        return (uu[6 * k + c] / n - (ru[4 * k + 1 + A[c]] / n) * (ru[4 * k + 1 + B[c]] / n)) * (s_u * s_u);
      });
    } else if (var == OUTPUT_DENSITY) {
      write4("MeanDensity", 1, [&](size_t k, int) { return (is_bb(k) ? (double)L->bb_rho : ru[4 * k] / n) * s_stress; });
    } else if (var == OUTPUT_SHEAR_STRESS) {
      pi = sums(HC_STATS_PI);
      const double factor = 0.5 * (double)L->omega - 1.0;
      write4("MeanShearStress", 6, [&](size_t k, int c) { return is_bb(k) ? 0.0 : factor * (pi[6 * k + c] / n) * s_stress; });
    } else if (var == OUTPUT_CELL_DENSITY) {
      for (unsigned int t = 0; t < h.cellfields->size(); t++) {
        const HemoCellField &cf = *(*h.cellfields)[t];
        const vector<long> dens = counts(HC_STATS_CELL_DENSITY, t), ins = counts(HC_STATS_INSIDE, t);
        const double s_d = si ? (double)cf.volumeFractionOfLspPerNode : 1.0;
        write4("CellDensity_" + cf.name, 1, [&](size_t k, int) { return (double)dens[k] / n * s_d; });
        write4("Hematocrit_" + cf.name, 1, [&](size_t k, int) { return (double)ins[k] / n; });
      }
    }
  }
  H5Fclose(file);
#else
  hlog << "(HemoCell) (FlowStatistics) built without HEMOCELL_WITH_HDF5: the means of " << ns << " samples are not written at " << h.iter << endl;
#endif
}

}  // namespace hemo
