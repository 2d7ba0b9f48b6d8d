// Time-averaged profiles from a short channel flow, with the running statistics of this back end (hemo::FlowStatistics,
// compat/flowStatistics.h): a 40 x 30 x 30 channel between two walls (z = 0 and z = nz - 1), periodic in x and y, two red cells
// and two platelets, a body force along x.  The sums are kept on the device and sampled every <statistics><every> iterations
// inside iterate(); nothing is downloaded until the end.
// Run it in a directory holding config.xml, RBC.xml, PLT.xml, RBC.pos and PLT.pos of tests/golden/statistics_case.
//
//   pipe_profile <config.xml> [tmax]
//
// At the end it writes <out>/hdf5/<iter>/Statistics.<iter>.p.0.h5 (HDF5 builds), prints the number of samples and the
// cross-stream profile of <u_x> and of the red cells' hematocrit, and dumps the raw sums to statistics_state.bin: the sample
// count, then the rho_u [n][4], uu [n][6] and pi [n][6] sums as doubles, then the vertex and inside counts [n] of the two types
// as 64-bit integers.
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "helper/flowStatistics.h"
#include "rbcHighOrderModel.h"
#include "pltSimpleModel.h"

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) { std::cout << "usage: " << argv[0] << " <config.xml> [tmax]" << std::endl; return 2; }
  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;
  const unsigned tmax = argc > 2 ? (unsigned)std::atoi(argv[2]) : (*cfg)["sim"]["tmax"].read<unsigned>();

  const plint nx = 40, ny = 30, nz = 30;
  param::lbm_base_parameters(*cfg);
  param::printParameters();
  const T force = (*cfg)["domain"]["drivingForce"].read<T>();

  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(
      defaultMultiBlockPolicy3D().getMultiBlockManagement(nx, ny, nz, 2), defaultMultiBlockPolicy3D().getBlockCommunicator(),
      defaultMultiBlockPolicy3D().getCombinedStatistics(), defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(),
      new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  hemocell.lattice->toggleInternalStatistics(false);
  defineDynamics(*hemocell.lattice, Box3D(0, nx - 1, 0, ny - 1, 0, 0), new BounceBack<T, DESCRIPTOR>(1.));
  defineDynamics(*hemocell.lattice, Box3D(0, nx - 1, 0, ny - 1, nz - 1, nz - 1), new BounceBack<T, DESCRIPTOR>(1.));
  hemocell.lattice->periodicity().toggleAll(false);
  hemocell.lattice->periodicity().toggle(0, true);
  hemocell.lattice->periodicity().toggle(1, true);
  hemocell.latticeEquilibrium(1., plb::Array<T, 3>(0., 0., 0.));
  hemocell.lattice->initialize();
  hemocell.outputInSiUnits = false;

  hemocell.initializeCellfield();
  hemocell.addCellType<RbcHighOrderModel>("RBC", RBC_FROM_SPHERE);
  hemocell.addCellType<PltSimpleModel>("PLT", ELLIPSOID_FROM_SPHERE);
  hemocell.setMaterialTimeScaleSeparation("RBC", (*cfg)["ibm"]["stepMaterialEvery"].read<int>());
  hemocell.setMaterialTimeScaleSeparation("PLT", (*cfg)["ibm"]["stepMaterialEvery"].read<int>());
  hemocell.setParticleVelocityUpdateTimeScaleSeparation((*cfg)["ibm"]["stepParticleEvery"].read<int>());
  hemocell.setOutputs("RBC", {OUTPUT_POSITION, OUTPUT_TRIANGLES});
  hemocell.setOutputs("PLT", {OUTPUT_POSITION, OUTPUT_TRIANGLES});
  hemocell.setFluidOutputs({OUTPUT_VELOCITY, OUTPUT_DENSITY, OUTPUT_SHEAR_STRESS, OUTPUT_CELL_DENSITY, OUTPUT_BOUNDARY});
  hemocell.loadParticles();

  FlowStatistics stats(hemocell);
  stats.enable((*cfg)["statistics"]["every"].read<unsigned>(), {OUTPUT_VELOCITY, OUTPUT_DENSITY, OUTPUT_SHEAR_STRESS, OUTPUT_CELL_DENSITY});

  const plb::Array<T, DESCRIPTOR<T>::d> F(force, 0.0, 0.0);
  setExternalVector(*hemocell.lattice, hemocell.lattice->getBoundingBox(), DESCRIPTOR<T>::ExternalField::forceBeginsAt, F);
  while (hemocell.iter < tmax) {
    hemocell.iterate();
    setExternalVector(*hemocell.lattice, hemocell.lattice->getBoundingBox(), DESCRIPTOR<T>::ExternalField::forceBeginsAt, F);
  }
  hemocell.writeOutput();
  stats.write();

  // the cross-stream profiles: means over the planes z = const of the fluid nodes' <u_x> and of the red cells' hematocrit
  const long ns = stats.samples();
  const size_t n = (size_t)nx * ny * nz;
  const vector<double> ru = stats.sums(HC_STATS_RHO_U), uu = stats.sums(HC_STATS_UU), pi = stats.sums(HC_STATS_PI);
  vector<vector<long>> counts;
  for (unsigned int t = 0; t < 2; t++) { counts.push_back(stats.counts(HC_STATS_CELL_DENSITY, t)); counts.push_back(stats.counts(HC_STATS_INSIDE, t)); }
  std::printf("SAMPLES %ld iteration %u\n", ns, hemocell.iter);
  for (plint z = 0; z < nz; z++) {
    double u = 0.0, hct = 0.0;
    const bool wall = z == 0 || z == nz - 1;   // a BounceBack node answers zero velocity, and nothing is inside a cell there
    for (plint x = 0; x < nx; x++) for (plint y = 0; y < ny; y++) {
      const size_t k = ((size_t)x * ny + y) * nz + z;
      if (!wall) u += ru[4 * k + 1] / (double)ns;
      hct += (double)counts[1][k] / (double)ns;
    }
    std::printf("PROFILE z %2ld  <u_x> %.6e  hematocrit_RBC %.4f\n", (long)z, u / (double)(nx * ny), hct / (double)(nx * ny));
  }
  std::FILE *o = std::fopen("statistics_state.bin", "wb");
  std::fwrite(&ns, sizeof(long), 1, o);
  std::fwrite(ru.data(), sizeof(double), ru.size(), o);
  std::fwrite(uu.data(), sizeof(double), uu.size(), o);
  std::fwrite(pi.data(), sizeof(double), pi.size(), o);
  for (const vector<long> &c : counts) std::fwrite(c.data(), sizeof(long), n, o);
  std::fclose(o);
  std::printf("DONE iteration %u samples %ld\n", hemocell.iter, ns);
  return 0;
}
