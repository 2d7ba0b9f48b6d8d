// Stretch of one stage V gametocyte (a malaria-infected red blood cell), driven through the source-level facade
// (hemocell_amd/compat) with RbcMalariaModel on a MESH_FROM_STL mesh.
// Inputs (tests/golden/malaria_case): config.xml (stretch force, dx, dt, tmax, tmeas), RBC_MALARIA.xml (the model, its
// <StlFile> and its inner edges), vRBC_uniform.stl (the cell's surface) and RBC_MALARIA.pos (one cell at 12 um, rotated
// by 90 degrees about x).  Box: 50^3 lattice nodes with no-slip walls; 19 vertices on each side of the cell are pulled
// apart along x with the configured force.  Prints one "(MalariaStretch)" line per measurement and writes stretch.log
// ("iter dx dy dz volume% surface% largest_diameter", lengths in um).
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "rbcMalariaModel.h"
#include "helper/cellInfo.h"
#include "helper/hemoCellStretch.h"

using namespace hemo;

int main(int argc, char *argv[]) {
  if (argc < 2) {
    cout << "Usage: " << argv[0] << " <configuration.xml>" << endl;
    return -1;
  }

  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;

  // ----------------- parameters ---------------------------------------------------------------
  param::lbm_base_parameters(*cfg);
  param::ef_lbm = (*cfg)["parameters"]["stretchForce"].read<T>() * 1e-12 / param::df;
  param::printParameters();
  const T to_um = 1e-6 / param::dx;
  const plint nx = 50, ny = 50, nz = 50;

  // ------------------------ lattice with no-slip walls ----------------------------------------
  pcout << "(MalariaStretch) Initializing lattice: " << nx << "x" << ny << "x" << nz << " [lu]" << std::endl;
  hemocell.lattice = new MultiBlockLattice3D<T, DESCRIPTOR>(
      defaultMultiBlockPolicy3D().getMultiBlockManagement(nx, ny, nz, 2), defaultMultiBlockPolicy3D().getBlockCommunicator(),
      defaultMultiBlockPolicy3D().getCombinedStatistics(), defaultMultiBlockPolicy3D().getMultiCellAccess<T, DESCRIPTOR>(),
      new GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0 / param::tau));
  hemocell.lattice->toggleInternalStatistics(false);
  hemocell.lattice->periodicity().toggleAll(false);
  OnLatticeBoundaryCondition3D<T, DESCRIPTOR> *boundaryCondition = createLocalBoundaryCondition3D<T, DESCRIPTOR>();
  boundaryCondition->setVelocityConditionOnBlockBoundaries(*hemocell.lattice);
  setBoundaryVelocity(*hemocell.lattice, hemocell.lattice->getBoundingBox(), plb::Array<T, 3>(0., 0., 0.));
  delete boundaryCondition;
  hemocell.latticeEquilibrium(1., hemo::Array<T, 3>({0., 0., 0.}));
  hemocell.lattice->initialize();

  // ----------------------- the gametocyte, its mesh read from the STL file -------------------
  hemocell.initializeCellfield();
  hemocell.addCellType<RbcMalariaModel>("RBC_MALARIA", MESH_FROM_STL);
  hemocell.setOutputs("RBC_MALARIA", {OUTPUT_POSITION, OUTPUT_TRIANGLES, OUTPUT_FORCE, OUTPUT_FORCE_INNER_LINK});
  hemocell.loadParticles();

  HemoCellField *cell = (*hemocell.cellfields)["RBC_MALARIA"];
  const unsigned int n_forced_lsps = 1 + 6 + 6 + 6;
  HemoCellStretch cellStretch(*cell, n_forced_lsps, param::ef_lbm);
  pcout << "(MalariaStretch) External stretching force [pN(flb)]: " << (*cfg)["parameters"]["stretchForce"].read<T>() << " ("
        << param::ef_lbm << ")" << endl;

  const T volume_eq = cell->meshmetric->getVolume() / std::pow(to_um, 3);
  const T surface_eq = cell->meshmetric->getSurface() / std::pow(to_um, 2);
  const unsigned int tmax = (*cfg)["sim"]["tmax"].read<unsigned int>();
  const unsigned int tmeas = (*cfg)["sim"]["tmeas"].read<unsigned int>();

  plb_ofstream fOut;
  fOut.open("stretch.log");
  while (hemocell.iter <= tmax) {
    if (hemocell.iter % tmeas == 0) {
      CellInformationFunctionals::calculateCellVolume(&hemocell);
      CellInformationFunctionals::calculateCellArea(&hemocell);
      CellInformationFunctionals::calculateCellStretch(&hemocell);
      CellInformationFunctionals::calculateCellBoundingBox(&hemocell);
      auto &ci = CellInformationFunctionals::info_per_cell[0];
      const T volume = ci.volume / std::pow(to_um, 3), surface = ci.area / std::pow(to_um, 2);
      const hemo::Array<T, 6> bbox = ci.bbox / to_um;
      const T largest_diam = ci.stretch / to_um;
      pcout << "(MalariaStretch) iter " << hemocell.iter << " diameters {" << bbox[1] - bbox[0] << ", " << bbox[3] - bbox[2] << ", "
            << bbox[5] - bbox[4] << "} um, volume " << volume / volume_eq * 100.0 << " %, surface " << surface / surface_eq * 100.0
            << " %" << endl;
      fOut << hemocell.iter << " " << bbox[1] - bbox[0] << " " << bbox[3] - bbox[2] << " " << bbox[5] - bbox[4] << " "
           << volume / volume_eq * 100.0 << " " << surface / surface_eq * 100.0 << " " << largest_diam << endl;
      CellInformationFunctionals::clear_list();
    }
    if (hemocell.iter == tmax) break;
    cellStretch.applyForce();   // not part of iterate(): applied by the driver every iteration
    hemocell.iterate();
  }
  fOut.close();

  pcout << "(MalariaStretch) Simulation finished :)" << std::endl;
  return 0;
}
