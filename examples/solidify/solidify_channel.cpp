// Solidify mechanics in a small channel (15 x 15 x 15 nodes, periodic along x and y) between a bounce-back floor with binding
// sites and a top wall moving in +x, with a few platelets above the floor, driven through the source-level facade
// (hemocell_amd/compat) with the names of the reference's drivers: a platelet that lies near a site once the shear has
// reached the floor is flagged, and turns into wall nodes and new binding sites at the next check.
// Run it in a directory holding config.xml, PLT.xml and a PLT.pos (tests/golden/solidify_case holds the reference's; the
// first platelet of that file reaches a wall node when rotated as its row says and is rejected at placement, as in the
// reference).
//
//   solidify_channel <config.xml> [tmax [save-at [output-at]]]
//
// save-at: saveCheckPoint at that iteration and stop; started with <out>/checkpoint/checkpoint.xml as configuration the run
// resumes from the dump.  output-at: one more writeOutput at that iteration.  At the end the fluid outputs are written (HDF5
// builds), and the populations, the mask, the binding field, the vertex positions and the vertex flags go to
// solidify_state.bin.
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "helper/hemocellInit.hh"
#include "pltSimpleModel.h"
#include "bindingField.h"

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) { std::cout << "usage: " << argv[0] << " <config.xml> [tmax [save-at [output-at]]]" << std::endl; return 2; }
  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;
  const unsigned tmax = argc > 2 ? (unsigned)std::atoi(argv[2]) : (*cfg)["sim"]["tmax"].read<unsigned>();
  const unsigned save_at = argc > 3 ? (unsigned)std::atoi(argv[3]) : 0;
  const unsigned output_at = argc > 4 ? (unsigned)std::atoi(argv[4]) : 0;

  const plint n = (*cfg)["domain"]["refDirN"].read<int>();
  const plint nx = n, ny = n, nz = n;
  param::lbm_pipe_parameters(*cfg, (int)n);
  param::printParameters();

  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(
      defaultMultiBlockPolicy3D().getMultiBlockManagement(nx, ny, nz, (*cfg)["domain"]["fluidEnvelope"].read<int>()),
      defaultMultiBlockPolicy3D().getBlockCommunicator(), defaultMultiBlockPolicy3D().getCombinedStatistics(),
      defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(), new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  hemocell.lattice->toggleInternalStatistics(false);
  hemocell.lattice->periodicity().toggle(0, true);
  hemocell.lattice->periodicity().toggle(1, true);
  hemocell.latticeEquilibrium(1., plb::Array<T, 3>(0., 0., 0.));

  // the top wall moves with the shear rate of the configuration times the height of the box
  const double u_top = (*cfg)["parameters"]["shearRate"].read<double>() * (double)nz * param::dx * (param::dt / param::dx);

  hemocell.initializeCellfield();
  hemocell.addCellType<PltSimpleModel>("PLT", ELLIPSOID_FROM_SPHERE);
  hemocell.setMaterialTimeScaleSeparation("PLT", (*cfg)["ibm"]["stepMaterialEvery"].read<int>());
  hemocell.enableSolidifyMechanics("PLT");
  hemocell.setSolidifyTimeScaleSeperation((*cfg)["ibm"]["stepParticleEvery"].read<int>());
  hemocell.setParticleVelocityUpdateTimeScaleSeparation((*cfg)["ibm"]["stepParticleEvery"].read<int>());
  hemocell.setOutputs("PLT", {OUTPUT_POSITION, OUTPUT_TRIANGLES});
  hemocell.setFluidOutputs({OUTPUT_VELOCITY, OUTPUT_BOUNDARY, OUTPUT_BINDING_SITES});
  hemocell.outputInSiUnits = false;

  Box3D topChannel(0, nx - 1, 0, ny - 1, nz - 1, nz - 1), bottomChannel(0, nx - 1, 0, ny - 1, 0, 0);
  OnLatticeBoundaryCondition3D<T, DESCRIPTOR> *boundaryCondition = createLocalBoundaryCondition3D<T, DESCRIPTOR>();
  boundaryCondition->setVelocityConditionOnBlockBoundaries(*hemocell.lattice, topChannel);
  setBoundaryVelocity(*hemocell.lattice, topChannel, plb::Array<T, 3>(u_top, 0, 0));
  defineDynamics(*hemocell.lattice, bottomChannel, new BounceBack<T, DESCRIPTOR>(1.));
  hemocell.lattice->initialize();

  Box3D bindingbox = bottomChannel;
  hemocell.cellfields->populateBindingSites(&bindingbox);

  if (!cfg->checkpointed) { hemocell.loadParticles(); hemocell.writeOutput(); }
  else hemocell.loadCheckPoint();

  while (hemocell.iter < tmax) {
    hemocell.iterate();
    if (save_at && hemocell.iter == save_at) { hemocell.saveCheckPoint(); return 0; }
    if (output_at && hemocell.iter == output_at) hemocell.writeOutput();
  }
  hemocell.writeOutput();

  // the state as the Python host would read it
  const size_t nn = (size_t)nx * ny * nz;
  std::vector<double> f(nn * HC_Q);
  std::vector<uint8_t> mask(nn), sites(nn);
  hc_lattice *L = hemocell.lattice->device();
  hc_check(hcl_download_populations(L, f.data()), "hcl_download_populations");
  hc_check(hcl_download_mask(L, mask.data()), "hcl_download_mask");
  hc_check(hcl_binding_download(L, sites.data()), "hcl_binding_download");
  hc_cells *C = hemocell.cellfields->device();
  long nv = 0, counts[3] = {0, 0, 0};
  hc_check(hcp_counts(C, &nv, nullptr, nullptr), "hcp_counts");
  std::vector<double> pos((size_t)nv * 3);
  std::vector<unsigned char> flags((size_t)nv);
  if (nv) { hc_check(hcp_download(C, 0, pos.data()), "hcp_download"); hc_check(hcp_solidify_flags_download(C, flags.data()), "hcp_solidify_flags_download"); }
  hc_check(hcp_solidify_counts(C, counts), "hcp_solidify_counts");
  std::FILE *o = std::fopen("solidify_state.bin", "wb");
  std::fwrite(f.data(), sizeof(double), f.size(), o);
  std::fwrite(mask.data(), 1, mask.size(), o);
  std::fwrite(sites.data(), 1, sites.size(), o);
  std::fwrite(pos.data(), sizeof(double), pos.size(), o);
  std::fwrite(flags.data(), 1, flags.size(), o);
  std::fclose(o);
  long walls = 0, nsites = 0;
  for (size_t k = 0; k < nn; k++) { walls += mask[k] != 0; nsites += sites[k] != 0; }
  std::printf("DONE iteration %u vertices %ld walls %ld sites %ld solidified_cells %ld solidified_nodes %ld flagged %ld\n", hemocell.iter, nv, walls, nsites,
              counts[0], counts[1], counts[2]);
  delete boundaryCondition;
  return 0;
}
