// HemoCellField::kernelMethod through the facade: the width of a cell type's IBM delta function.
//   ibm_kernel_driver phi2|phi3|phi4|both <config.xml> [iterations]
// One RBC (RBC.xml, RBC.pos of tests/golden/shear_case) in a periodic 40 x 30 x 30 box under a body force written after every
// iteration, as the shipped drivers write it.  phi3 / phi4 assign interpolationCoefficientsPhi3 / ...Phi4 to the type's
// kernelMethod before the particles are loaded; `both` assigns one after the other (the last one counts).  At the end the
// kernel the library holds for the type is printed, and the post-stream populations and the vertex positions go to
// ibm_kernel_state.bin for a comparison with the same run on the Python host.
#include "hemocell.h"
#include "rbcHighOrderModel.h"
#include <cstring>

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 3) { std::cout << "usage: ibm_kernel_driver phi2|phi3|phi4|both config.xml [iterations]" << std::endl; return 2; }
  const std::string mode = argv[1];
  const int tmax = argc > 3 ? std::atoi(argv[3]) : 20;
  HemoCell hemocell(argv[2], argc, argv);
  Config *cfg = hemocell.cfg;
  param::lbm_base_parameters(*cfg);
  const plint nx = 40, ny = 30, nz = 30;
  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(defaultMultiBlockPolicy3D().getMultiBlockManagement(nx, ny, nz, 1),
                                                            defaultMultiBlockPolicy3D().getBlockCommunicator(), defaultMultiBlockPolicy3D().getCombinedStatistics(),
                                                            defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(),
                                                            new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  hemocell.lattice->toggleInternalStatistics(false);
  hemocell.lattice->periodicity().toggleAll(true);
  hemocell.latticeEquilibrium(1., hemo::Array<T, 3>({0., 0., 0.}));
  hemocell.lattice->initialize();
  hemocell.initializeCellfield();
  hemocell.addCellType<RbcHighOrderModel>("RBC", RBC_FROM_SPHERE);
  hemocell.setMaterialTimeScaleSeparation("RBC", 1);
  hemocell.setParticleVelocityUpdateTimeScaleSeparation(2);
  HemoCellField &field = *(*hemocell.cellfields)["RBC"];
  if (mode == "phi3" || mode == "both") field.kernelMethod = interpolationCoefficientsPhi3;
  if (mode == "phi4" || mode == "both") field.kernelMethod = interpolationCoefficientsPhi4;
  if (mode == "phi2") field.kernelMethod = interpolationCoefficientsPhi2;
  hemocell.loadParticles();
  const T F = 2e-5;
  setExternalVector(*hemocell.lattice, hemocell.lattice->getBoundingBox(), DESCRIPTOR<T>::ExternalField::forceBeginsAt, plb::Array<T, 3>(F, 0., -F / 2));
  for (int it = 0; it < tmax; it++) {
    hemocell.iterate();
    setExternalVector(*hemocell.lattice, hemocell.lattice->getBoundingBox(), DESCRIPTOR<T>::ExternalField::forceBeginsAt, plb::Array<T, 3>(F, 0., -F / 2));
  }
  hc_lattice *L = hemocell.lattice->device();
  hc_cells *C = hemocell.cellfields->device();
  int kernel = 0;
  hc_check(hcp_type_get_ibm_kernel(C, 0, &kernel), "hcp_type_get_ibm_kernel");
  std::vector<double> f((size_t)nx * ny * nz * HC_Q);
  hc_check(hcl_download_populations(L, f.data()), "hcl_download_populations");
  long nv = 0;
  hc_check(hcp_counts(C, &nv, nullptr, nullptr), "hcp_counts");
  std::vector<double> pos((size_t)nv * 3);
  hc_check(hcp_download(C, 0, pos.data()), "hcp_download");
  std::FILE *o = std::fopen("ibm_kernel_state.bin", "wb");
  std::fwrite(f.data(), sizeof(double), f.size(), o);
  std::fwrite(pos.data(), sizeof(double), pos.size(), o);
  std::fclose(o);
  std::printf("DONE iteration %u vertices %ld kernel %d\n", hemocell.iter, nv, kernel);
  return 0;
}
