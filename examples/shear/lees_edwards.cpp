// Simple shear between Lees-Edwards boundaries on the z faces of a small fully periodic box with a few RBCs, driven through
// the source-level facade (hemocell_amd/compat) the way the reference's cases/leesEdwards driver is written.
// Run it in a directory holding config.xml (examples/shear), RBC_HO.pos and RBC_HO.xml (tests/golden/lees_edwards_case).
//
//   lees_edwards <config.xml> [update-every [tmax [save-at]]]
//
// update-every: after every iterate() the driver calls LEbc.updateLECurDisplacement(iter) when iter % update-every == 0
// (1 = the reference's pattern, 0 = never).  save-at: saveCheckPoint at that iteration.  Started with
// <out>/checkpoint/checkpoint.xml as configuration the run resumes from the dump.  A fourth argument "particle-shift" sets
// hemocell.leesEdwardsBC, which the back end refuses.  At the end the post-stream populations and the vertex positions are
// written to le_state.bin.
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "helper/leesEdwardsBC.h"
#include "rbcHighOrderModel.h"

#include <cstring>

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) { std::cout << "usage: " << argv[0] << " <config.xml> [update-every [tmax [save-at]]]" << std::endl; return 2; }
  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;
  const unsigned update_every = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1;
  unsigned tmax = argc > 3 ? (unsigned)std::atoi(argv[3]) : (*cfg)["sim"]["tmax"].read<unsigned>();
  const bool particle_shift = argc > 4 && std::strcmp(argv[4], "particle-shift") == 0;
  const unsigned save_at = argc > 4 && !particle_shift ? (unsigned)std::atoi(argv[4]) : 0;

  const plint n = (*cfg)["domain"]["boxSize"].read<plint>();
  const double dt = (*cfg)["domain"]["dt"].read<double>();
  param::lbm_shear_parameters(*cfg, n);
  param::printParameters();

  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(
      defaultMultiBlockPolicy3D().getMultiBlockManagement(n, n, n, 2), defaultMultiBlockPolicy3D().getBlockCommunicator(),
      defaultMultiBlockPolicy3D().getCombinedStatistics(), defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(),
      new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  hemocell.lattice->toggleInternalStatistics(false);
  LeesEdwardsBC<T, DESCRIPTOR> LEbc(*hemocell.lattice, param::shearrate_lbm, dt, &hemocell.LEcurrentDisplacement);
  LEbc.initialize();
  hemocell.lattice->initialize();
  hemocell.leesEdwardsBC = particle_shift;

  hemocell.initializeCellfield();
  hemocell.addCellType<RbcHighOrderModel>("RBC_HO", RBC_FROM_SPHERE);
  hemocell.setMaterialTimeScaleSeparation("RBC_HO", 20);
  hemocell.setParticleVelocityUpdateTimeScaleSeparation(5);

  if (!cfg->checkpointed) hemocell.loadParticles();
  else {
    hemocell.loadCheckPoint();
    LEbc.updateLECurDisplacement(hemocell.iter);   // the displacement belongs to the driver: set it again for the resumed iteration
  }

  if (hemocell.iter == 0)
    for (plint i = 0; i < (*cfg)["parameters"]["warmup"].read<plint>(); ++i) hemocell.lattice->collideAndStream();

  while (hemocell.iter < tmax) {
    hemocell.iterate();
    if (update_every && hemocell.iter % update_every == 0) LEbc.updateLECurDisplacement(hemocell.iter);
    if (save_at && hemocell.iter == save_at) { hemocell.saveCheckPoint(); return 0; }
  }

  // the state as the Python host would read it: post-stream populations, then the vertex positions
  hc_lattice *L = hemocell.lattice->device();
  hc_cells *C = hemocell.cellfields->device();
  std::vector<double> f((size_t)n * n * n * HC_Q);
  hc_check(hcl_download_populations(L, f.data()), "hcl_download_populations");
  long nv = 0;
  hc_check(hcp_counts(C, &nv, nullptr, nullptr), "hcp_counts");
  std::vector<double> pos((size_t)nv * 3);
  hc_check(hcp_download(C, 0, pos.data()), "hcp_download");
  std::FILE *o = std::fopen("le_state.bin", "wb");
  std::fwrite(f.data(), sizeof(double), f.size(), o);
  std::fwrite(pos.data(), sizeof(double), pos.size(), o);
  std::fclose(o);
  std::printf("DONE iteration %u vertices %ld D %.17g\n", hemocell.iter, nv, LeesEdwardsBC<T, DESCRIPTOR>::LEcurrentDisplacement);
  return 0;
}
