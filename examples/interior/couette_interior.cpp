// One RBC with a viscous interior in a Couette box (50 x 50 x 30 nodes between two walls moving in +-x), driven through the
// source-level facade (hemocell_amd/compat) the way the reference's examples/cellCollision_interior_viscosity driver is written.
// Run it in a directory holding config.xml, RBC.xml and RBC.pos of tests/golden/interior_viscosity_case: RBC.xml carries
// <enableInteriorViscosity> and <viscosityRatio>, config.xml the two cadences <sim><interiorViscosity> and
// <interiorViscosityEntireGrid>.
//
//   couette_interior <config.xml> [tmax [save-at [membrane-every entire-grid-every]]]
//
// save-at: saveCheckPoint at that iteration and stop; started with <out>/checkpoint/checkpoint.xml as configuration the run
// resumes from the dump.  The two last arguments replace the cadences of the configuration.  At the end the fluid fields
// Velocity, Omega and InteriorPoints are written (HDF5 builds), and the post-stream populations, the vertex positions and the
// class byte of every node go to interior_state.bin, and a PASSES line tells how often each pass ran in this process.
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "helper/hemocellInit.hh"
#include "rbcHighOrderModel.h"

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) { std::cout << "usage: " << argv[0] << " <config.xml> [tmax [save-at [membrane-every entire-grid-every]]]" << std::endl; return 2; }
  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;
  const unsigned tmax = argc > 2 ? (unsigned)std::atoi(argv[2]) : (*cfg)["sim"]["tmax"].read<unsigned>();
  const unsigned save_at = argc > 3 ? (unsigned)std::atoi(argv[3]) : 0;

  const plint nx = 50, ny = 50, nz = 30;
  param::lbm_shear_parameters(*cfg, ny);
  param::printParameters();

  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(
      defaultMultiBlockPolicy3D().getMultiBlockManagement(nx, ny, nz, 2), defaultMultiBlockPolicy3D().getBlockCommunicator(),
      defaultMultiBlockPolicy3D().getCombinedStatistics(), defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(),
      new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  OnLatticeBoundaryCondition3D<T, DESCRIPTOR> *boundaryCondition = createLocalBoundaryCondition3D<T, DESCRIPTOR>();
  hemocell.lattice->toggleInternalStatistics(false);
  iniLatticeSquareCouette(*hemocell.lattice, nx, ny, nz, *boundaryCondition, param::shearrate_lbm);
  hemocell.lattice->initialize();
  hemocell.outputInSiUnits = false;   // Omega and InteriorPoints as the lattice holds them

  hemocell.initializeCellfield();
  hemocell.addCellType<RbcHighOrderModel>("RBC", RBC_FROM_SPHERE);
  hemocell.setOutputs("RBC", {OUTPUT_POSITION, OUTPUT_TRIANGLES});
  hemocell.setFluidOutputs({OUTPUT_VELOCITY, OUTPUT_OMEGA, OUTPUT_INTERIOR_POINTS});
  hemocell.setParticleVelocityUpdateTimeScaleSeparation(5);
  if (argc > 5) hemocell.setInteriorViscosityTimeScaleSeperation((unsigned)std::atoi(argv[4]), (unsigned)std::atoi(argv[5]));
  else hemocell.setInteriorViscosityTimeScaleSeperation((*cfg)["sim"]["interiorViscosity"].read<int>(), (*cfg)["sim"]["interiorViscosityEntireGrid"].read<int>());

  if (!cfg->checkpointed) hemocell.loadParticles();
  else hemocell.loadCheckPoint();
  hc_check(hc_profile_enable(1), "hc_profile_enable");   // counts the passes this process runs (reported below)

  while (hemocell.iter < tmax) {
    hemocell.iterate();
    if (save_at && hemocell.iter == save_at) { hemocell.saveCheckPoint(); return 0; }
  }
  hemocell.writeOutput();

  // the state as the Python host would read it
  hc_lattice *L = hemocell.lattice->device();
  hc_cells *C = hemocell.cellfields->device();
  const size_t n = (size_t)nx * ny * nz;
  std::vector<double> f(n * HC_Q);
  hc_check(hcl_download_populations(L, f.data()), "hcl_download_populations");
  long nv = 0;
  hc_check(hcp_counts(C, &nv, nullptr, nullptr), "hcp_counts");
  std::vector<double> pos((size_t)nv * 3);
  hc_check(hcp_download(C, 0, pos.data()), "hcp_download");
  std::vector<uint8_t> cls(n);
  hc_check(hcl_interior_download_classes(L, cls.data()), "hcl_interior_download_classes");
  long tagged = 0;
  for (uint8_t c : cls) tagged += c != 0;
  std::FILE *o = std::fopen("interior_state.bin", "wb");
  std::fwrite(f.data(), sizeof(double), f.size(), o);
  std::fwrite(pos.data(), sizeof(double), pos.size(), o);
  std::fwrite(cls.data(), 1, cls.size(), o);
  std::fclose(o);
  double ms = 0; long n_find = 0, n_membrane = 0;
  hc_check(hc_profile_read("interior_find", &ms, &n_find), "hc_profile_read");
  hc_check(hc_profile_read("interior_membrane", &ms, &n_membrane), "hc_profile_read");
  std::printf("PASSES entire-grid %ld membrane %ld\n", n_find, n_membrane);
  std::printf("DONE iteration %u vertices %ld tagged %ld tau_int %.17g\n", hemocell.iter, nv, tagged, (*hemocell.cellfields)["RBC"]->interiorViscosityTau);
  return 0;
}
