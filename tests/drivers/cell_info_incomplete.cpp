// CellInformationFunctionals and writeCellInfo_CSV (helper/cellInfo.cpp, io/writeCellInfoCSV.cpp) with one complete cell and one
// that has lost particles at the pipe wall (core/hemoCellParticleField.cpp:304-321, "particle" deletion mode), printed for
// tests/test_gpu_observables.py to check against tests/observables_ref.py:
//   TRI <a> <b> <c>                               the RBC mesh
//   V <cell id> <vertex> <alive> x y z vx vy vz      every stored particle before any call
//   INFO <id> volume area x y z stretch vx vy vz x0 x1 y0 y1 z0 z1   calculateCellInformation(hemocell, map)
//   CSV <path>                                    the file writeCellInfo_CSV wrote
//   STRETCH <id> s / POSITION <id> x y z           calculateCellStretch / calculateCellPosition, in that order
//   CELLS <n>                                     cells left afterwards
#ifndef HEMOCELL_COMPAT_MAIN
#define HEMOCELL_COMPAT_MAIN
#endif
#include "hemocell.h"
#include "rbcHighOrderModel.h"

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) { cout << "Usage: " << argv[0] << " <configuration.xml>" << endl; return -1; }
  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;
  param::lbm_base_parameters(*cfg);
  const plint nx = 96, ny = 34, nz = 34;
  std::unique_ptr<MultiScalarField3D<int>> flagMatrix;
  std::unique_ptr<VoxelizedDomain3D<T>> voxelizedDomain;
  getFlagMatrixCylinder(nx, ny, nz, voxelizedDomain, flagMatrix);
  hemocell.initializeLattice(voxelizedDomain->getMultiBlockManagement());
  defineDynamics(*hemocell.lattice, *flagMatrix, hemocell.lattice->getBoundingBox(), new BounceBack<T, DESCRIPTOR>(1.), 0);
  hemocell.lattice->toggleInternalStatistics(false);
  hemocell.lattice->periodicity().toggleAll(false);
  hemocell.latticeEquilibrium(1., plb::Array<T, 3>(0., 0., 0.));
  hemocell.lattice->initialize();
  hemocell.initializeCellfield();
  hemocell.addCellType<RbcHighOrderModel>("RBC", RBC_FROM_SPHERE);
  hemocell.setMaterialTimeScaleSeparation("RBC", 4);
  hemocell.setParticleVelocityUpdateTimeScaleSeparation(60);
  hemocell.setOutputs("RBC", {OUTPUT_POSITION});
  hemocell.setFluidOutputs({OUTPUT_VELOCITY});
  hemocell.setSystemPeriodicity(0, true);
  hemocell.loadParticles();
  hemocell.iterate();                                       // iteration 0 interpolates; velocities are then held for 60 iterations
  hc_cells *c = hemocell.cellfields->device();
  long nv = 0, nc = 0, inc = 0;
  hcp_counts(c, &nv, &nc, nullptr);
  vector<double> vel((size_t)(3 * nv));
  hc_check(hcp_download(c, 1, vel.data()), "hcp_download");
  for (long i = nv / 2; i < nv; i++) { vel[3 * i] = 0.01; vel[3 * i + 1] = -0.002; vel[3 * i + 2] = 0.1; }   // cell 1 towards the wall
  hc_check(hcp_upload(c, 1, vel.data()), "hcp_upload");
  for (int i = 0; i < 55 && inc == 0; i++) {               // up to the first particles lost: the cell is listed, incomplete
    hemocell.iterate();
    c = hemocell.cellfields->device();
    hcp_deletion_counts(c, nullptr, nullptr, &inc, nullptr);
  }
  c = hemocell.cellfields->device();
  hcp_counts(c, &nv, &nc, nullptr);
  std::printf("STATE iteration %u cells %ld incomplete %ld\n", hemocell.iter, nc, inc);
  for (const auto &t : (*hemocell.cellfields)["RBC"]->triangle_list) std::printf("TRI %ld %ld %ld\n", (long)t[0], (long)t[1], (long)t[2]);
  vector<double> pos((size_t)(3 * nv)); vel.assign((size_t)(3 * nv), 0.0);
  vector<unsigned char> alive((size_t)nv); vector<long> ids((size_t)nc);
  hc_check(hcp_download(c, 0, pos.data()), "hcp_download"); hc_check(hcp_download(c, 1, vel.data()), "hcp_download");
  hc_check(hcp_download_alive(c, alive.data()), "hcp_download_alive"); hc_check(hcp_download_cell_ids(c, ids.data()), "hcp_download_cell_ids");
  const long per = nv / nc;
  for (long i = 0; i < nv; i++)
    std::printf("V %ld %ld %d %.17g %.17g %.17g %.17g %.17g %.17g\n", ids[(size_t)(i / per)], i % per, (int)alive[(size_t)i], pos[3 * i], pos[3 * i + 1], pos[3 * i + 2],
                vel[3 * i], vel[3 * i + 1], vel[3 * i + 2]);
  map<int, CellInformation> info;
  CellInformationFunctionals::calculateCellInformation(&hemocell, info);
  for (const auto &kv : info) {
    const CellInformation &ci = kv.second;
    std::printf("INFO %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", kv.first, ci.volume, ci.area, ci.position[0], ci.position[1], ci.position[2], ci.stretch,
                ci.velocity[0], ci.velocity[1], ci.velocity[2]);
    for (int d = 0; d < 6; d++) std::printf(" %.17g", ci.bbox[d]);
    std::printf("\n");
  }
  hemocell.outputInSiUnits = false;
  ::mkdir(hemocell.outDir.c_str(), 0777);
  writeCellInfo_CSV(hemocell);
  char it[32]; std::snprintf(it, sizeof(it), "%012u", hemocell.iter);
  std::printf("CSV %s/csv/RBC.%s.csv\n", hemocell.outDir.c_str(), it);
  CellInformationFunctionals::clear_list();
  CellInformationFunctionals::calculateCellStretch(&hemocell);
  for (const auto &kv : CellInformationFunctionals::info()) std::printf("STRETCH %d %.17g\n", kv.first, kv.second.stretch);
  CellInformationFunctionals::clear_list();
  CellInformationFunctionals::calculateCellPosition(&hemocell);
  for (const auto &kv : CellInformationFunctionals::info())
    std::printf("POSITION %d %.17g %.17g %.17g\n", kv.first, kv.second.position[0], kv.second.position[1], kv.second.position[2]);
  CellInformationFunctionals::clear_list();
  hcp_counts(hemocell.cellfields->device(), nullptr, &nc, nullptr);
  std::printf("CELLS %ld\n", nc);
  return 0;
}
