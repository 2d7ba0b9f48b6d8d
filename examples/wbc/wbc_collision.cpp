// Two white blood cells passing each other in a Couette shear box, driven through the source-level facade
// (hemocell_amd/compat) with WbcHighOrderModel on WBC_SPHERE meshes.
// Inputs (tests/golden/wbc_case): config.xml (shear rate, dx, dt, tmax, tmeas), WBC_HO.xml (the model, its
// rigid-core and cytoskeleton constants and its inner edges) and WBC_HO.pos (one cell below and one above the
// zero-velocity mid-plane, 15 um apart in x and 6 um apart in z, so that their paths cross).
// Box: 30 x 12 x 18 um, periodic in x and y, walls at z = 0 (moving in +x) and z = nz-1 (moving in -x).
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "wbcHighOrderModel.h"
#include "helper/hemocellInit.hh"
#include "helper/cellInfo.h"

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) {
    cout << "Usage: " << argv[0] << " <configuration.xml>" << endl;
    return -1;
  }

  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;

  // ----------------- parameters: the wall distance sets the shear scale ----------------------
  pcout << "(WbcCollision) (Parameters) calculating shear flow parameters" << endl;
  const T to_lu = 1e-6 / (*cfg)["domain"]["dx"].read<T>();
  const plint nx = 30 * to_lu, ny = 12 * to_lu, nz = 18 * to_lu;
  param::lbm_shear_parameters(*cfg, nz);
  param::printParameters();

  // ------------------------ lattice and the moving walls -------------------------------------
  pcout << "(WbcCollision) Initializing lattice: " << nx << "x" << ny << "x" << nz << " [lu]" << std::endl;
  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(
      defaultMultiBlockPolicy3D().getMultiBlockManagement(nx, ny, nz, 2), defaultMultiBlockPolicy3D().getBlockCommunicator(),
      defaultMultiBlockPolicy3D().getCombinedStatistics(), defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(),
      new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  OnLatticeBoundaryCondition3D<T, DESCRIPTOR> *boundaryCondition = createLocalBoundaryCondition3D<T, DESCRIPTOR>();
  hemocell.lattice->toggleInternalStatistics(false);
  iniLatticeSquareCouette(*hemocell.lattice, nx, ny, nz, *boundaryCondition, param::shearrate_lbm);
  hemocell.lattice->initialize();
  delete boundaryCondition;

  // ----------------------- the white blood cells --------------------------------------------
  hemocell.initializeCellfield();
  hemocell.addCellType<WbcHighOrderModel>("WBC_HO", WBC_SPHERE);
  hemocell.setOutputs("WBC_HO", {OUTPUT_POSITION, OUTPUT_TRIANGLES, OUTPUT_FORCE, OUTPUT_FORCE_INNER_LINK});
  hemocell.setFluidOutputs({OUTPUT_VELOCITY});
  hemocell.loadParticles();
  hemocell.writeOutput();

  pcout << "(WbcCollision) Shear rate: " << (*cfg)["domain"]["shearrate"].read<T>() << " s^-1." << endl;
  const unsigned int tmax = (*cfg)["sim"]["tmax"].read<unsigned int>();
  const unsigned int tmeas = (*cfg)["sim"]["tmeas"].read<unsigned int>();

  while (hemocell.iter < tmax) {
    hemocell.iterate();
    if (hemocell.iter % tmeas == 0) {
      hemocell.writeOutput();
      CellInformationFunctionals::calculateCellInformation(&hemocell);
      for (auto &kv : CellInformationFunctionals::info())
        pcout << "(WbcCollision) iter " << hemocell.iter << " cell " << kv.first << " centre x " << kv.second.position[0] / to_lu
              << " um, z " << kv.second.position[2] / to_lu << " um" << endl;
      CellInformationFunctionals::clear_list();
    }
  }

  pcout << "(WbcCollision) Simulation finished :)" << std::endl;
  return 0;
}
