// A cylinder fed by a pre-inlet, driven through the source-level facade (hemocell_amd/compat) the way the reference's
// examples/pipeflow_with_preinlet is written -- with an analytic cylinder instead of an STL, so the walls come from
// defineDynamics with a DomainFunctional3D and the pre-inlet from the constructor that reads the lattice's walls.
// Run it in a directory holding the files of tests/golden/preinlet_facade_case (config.xml, RBC.xml, PLT.xml, RBC.pos,
// PLT.pos, pulse.dat).
//
//   pipe_with_preinlet <config.xml> [key=value ...]
//
// direction=Xneg|Xpos|Yneg|Ypos|Zneg|Zpos (Xneg)   the side the pre-inlet lies on; the cylinder runs along that axis
// nx= ny= nz=                                        the domain (default <domain><nx|ny|nz>)
// tmax=                                              iterations (default <sim><tmax>)
// cells=0                                            fluid only: no cell types, no particles
// pulse=1                                            readNormalizedVelocities(): the pulsatile driving force
// dump=1                                             after iterations 1 and tmax write preinlet_dump.<iter>.bin: both lattices'
//                                                    populations and both containers' particle records, read through the C ABI
// output=1                                           writeOutput() at the end
// timing=K                                           print the wall time per iteration of the iterations after the first K
// checkpoint=save|load, twice=1                      saveCheckPoint() twice at the end / loadCheckPoint() / declare a node twice
#define HEMOCELL_COMPAT_MAIN
#include "hemocell.h"
#include "rbcHighOrderModel.h"
#include "pltSimpleModel.h"
#include "cellInfo.h"
#include "fluidInfo.h"
#include "preInlet.h"

#include <chrono>
#include <cstring>

using namespace hemo;

// the wall of a cylinder of radius R along `axis` through the middle of the box
class CylinderWall : public DomainFunctional3D {
 public:
  CylinderWall(int axis_, T c0_, T c1_, T R_) : axis(axis_), c0(c0_), c1(c1_), R(R_) {}
  bool operator()(plint iX, plint iY, plint iZ) const override {
    const T a = axis == 0 ? iY : iX, b = axis == 2 ? iY : iZ;
    return (a - c0) * (a - c0) + (b - c1) * (b - c1) > R * R;
  }
  CylinderWall *clone() const override { return new CylinderWall(*this); }
 private:
  int axis; T c0, c1, R;
};

static void dump(HemoCell &hemocell) {
  PreInlet &p = *hemocell.preInlet;
  hc_lattice *L[2] = {hemocell.lattice->device(), p.lattice->device_now()};
  hc_cells *C[2] = {hemocell.cellfields->device(), p.cells};
  const long nodes[2] = {(long)(hemocell.lattice->nx * hemocell.lattice->ny * hemocell.lattice->nz), (long)(p.lattice->nx * p.lattice->ny * p.lattice->nz)};
  long nrec[2] = {0, 0};
  std::vector<double> f[2]; std::vector<HemoCellParticle::serializeValues_t> rec[2];
  for (int k = 0; k < 2; k++) {
    f[k].resize((size_t)nodes[k] * HC_Q);
    hc_check(hcl_download_populations(L[k], f[k].data()), "hcl_download_populations");
    if (!C[k]) continue;
    long nvt = 0, miss = 0;
    hc_check(hcp_counts(C[k], &nvt, nullptr, nullptr), "hcp_counts"); hc_check(hcp_deletion_counts(C[k], nullptr, nullptr, nullptr, &miss), "hcp_deletion_counts");
    nrec[k] = nvt - miss; rec[k].resize((size_t)nrec[k]);
    if (nrec[k]) hc_check(hcp_download_records(C[k], rec[k].data(), nrec[k]), "hcp_download_records");
  }
  const string name = "preinlet_dump." + std::to_string(hemocell.iter) + ".bin";
  std::FILE *o = std::fopen(name.c_str(), "wb");
  const long hdr[4] = {nodes[0], nodes[1], nrec[0], nrec[1]};
  std::fwrite(hdr, sizeof(long), 4, o);
  for (int k = 0; k < 2; k++) std::fwrite(f[k].data(), sizeof(double), f[k].size(), o);
  for (int k = 0; k < 2; k++) std::fwrite(rec[k].data(), sizeof(rec[k][0]), rec[k].size(), o);
  std::fclose(o);
}

int main(int argc, char *argv[]) {
  if (argc < 2) { cout << "Usage: " << argv[0] << " <configuration.xml> [key=value ...]" << endl; return -1; }
  HemoCell hemocell(argv[1], argc, argv);
  Config *cfg = hemocell.cfg;
  std::map<string, string> opt;
  for (int i = 2; i < argc; i++) { const char *eq = std::strchr(argv[i], '='); if (eq) opt[string((const char *)argv[i], (size_t)(eq - argv[i]))] = string(eq + 1); }
  auto number = [&](const char *key, long fallback) { return opt.count(key) ? std::atol(opt[key].c_str()) : fallback; };
  const std::map<string, Direction> directions = {{"Xpos", Xpos}, {"Xneg", Xneg}, {"Ypos", Ypos}, {"Yneg", Yneg}, {"Zpos", Zpos}, {"Zneg", Zneg}};
  const string dname = opt.count("direction") ? opt["direction"] : "Xneg";
  if (!directions.count(dname)) { cout << "unknown direction " << dname << endl; return -1; }
  const Direction direction = directions.at(dname);
  const int axis = (direction == Xpos || direction == Xneg) ? 0 : (direction == Ypos || direction == Yneg) ? 1 : 2;
  const bool neg = direction == Xneg || direction == Yneg || direction == Zneg;
  const plint n[3] = {number("nx", (*cfg)["domain"]["nx"].read<plint>()), number("ny", (*cfg)["domain"]["ny"].read<plint>()), number("nz", (*cfg)["domain"]["nz"].read<plint>())};
  const unsigned int tmax = (unsigned int)number("tmax", (*cfg)["sim"]["tmax"].read<long>());
  const bool with_cells = number("cells", 1) != 0, do_dump = number("dump", 0) != 0;

  hlog << "(PipePreInlet) (Parameters) setting lbm parameters" << endl;
  param::lbm_base_parameters(*cfg);
  param::printParameters();

  hlog << "(PipePreInlet) (Fluid) Initializing the fluid field: a cylinder along axis " << axis << endl;
  MultiBlockManagement3D management = defaultMultiBlockPolicy3D().getMultiBlockManagement(n[0], n[1], n[2], 1);
  hemocell.initializeLattice(management);
  hemocell.lattice->periodicity().toggleAll(false);
  const plint na = n[axis == 0 ? 1 : 0], nb = n[axis == 2 ? 1 : 2];
  defineDynamics(*hemocell.lattice, hemocell.lattice->getBoundingBox(), new CylinderWall(axis, (na - 1) / 2.0, (nb - 1) / 2.0, (std::min(na, nb) - 2) / 2.0),
                 new BounceBack<T, DESCRIPTOR>(1.));

  hlog << "(PipePreInlet) (PreInlets) creating preInlet " << dname << endl;
  hemocell.preInlet = new hemo::PreInlet(&hemocell, management);
  Box3D slice = hemocell.lattice->getBoundingBox();
  if (axis == 0) { if (neg) slice.x1 = slice.x0; else slice.x0 = slice.x1; }
  if (axis == 1) { if (neg) slice.y1 = slice.y0; else slice.y0 = slice.y1; }
  if (axis == 2) { if (neg) slice.z1 = slice.z0; else slice.z0 = slice.z1; }
  hemocell.preInlet->preInletFromSlice(direction, slice);
  hemocell.preInlet->initializePreInlet();
  hemocell.preInlet->createBoundary();
  const Box3D loc = hemocell.preInlet->location;
  hlog << "(PipePreInlet) (PreInlets) location " << loc.x0 << " " << loc.x1 << " " << loc.y0 << " " << loc.y1 << " " << loc.z0 << " " << loc.z1 << endl;

  hemocell.lattice->toggleInternalStatistics(false);
  hemocell.latticeEquilibrium(1., plb::Array<double, 3>(0., 0., 0.));
  hemocell.preInlet->calculateDrivingForce();
  if (number("pulse", 0) && !hemocell.preInlet->readNormalizedVelocities()) return -1;
  hemocell.lattice->initialize();

  hemocell.initializeCellfield();
  if (with_cells) {
    hemocell.addCellType<RbcHighOrderModel>("RBC", RBC_FROM_SPHERE);
    hemocell.setMaterialTimeScaleSeparation("RBC", (*cfg)["ibm"]["stepMaterialEvery"].read<int>());
    hemocell.addCellType<PltSimpleModel>("PLT", ELLIPSOID_FROM_SPHERE);
    hemocell.setMaterialTimeScaleSeparation("PLT", (*cfg)["ibm"]["stepMaterialEvery"].read<int>());
    hemocell.setParticleVelocityUpdateTimeScaleSeparation((*cfg)["ibm"]["stepParticleEvery"].read<int>());
    hemocell.setOutputs("RBC", {OUTPUT_POSITION, OUTPUT_TRIANGLES, OUTPUT_FORCE});
    hemocell.setOutputs("PLT", {OUTPUT_POSITION, OUTPUT_TRIANGLES, OUTPUT_FORCE});
  }
  hemocell.setFluidOutputs({OUTPUT_VELOCITY, OUTPUT_DENSITY, OUTPUT_FORCE, OUTPUT_BOUNDARY});

  // the outlet: a pressure plane on the face opposite the inlet
  {
    Box3D outlet = hemocell.lattice->getBoundingBox();
    OnLatticeBoundaryCondition3D<T, DESCRIPTOR> *boundary = new BoundaryConditionInstantiator3D<T, DESCRIPTOR, WrappedZouHeBoundaryManager3D<T, DESCRIPTOR>>();
    if (axis == 0) { if (neg) { outlet.x0 = outlet.x1; boundary->addPressureBoundary0P(outlet, *hemocell.lattice, boundary::density); } else { outlet.x1 = outlet.x0; boundary->addPressureBoundary0N(outlet, *hemocell.lattice, boundary::density); } }
    if (axis == 1) { if (neg) { outlet.y0 = outlet.y1; boundary->addPressureBoundary1P(outlet, *hemocell.lattice, boundary::density); } else { outlet.y1 = outlet.y0; boundary->addPressureBoundary1N(outlet, *hemocell.lattice, boundary::density); } }
    if (axis == 2) { if (neg) { outlet.z0 = outlet.z1; boundary->addPressureBoundary2P(outlet, *hemocell.lattice, boundary::density); } else { outlet.z1 = outlet.z0; boundary->addPressureBoundary2N(outlet, *hemocell.lattice, boundary::density); } }
    setBoundaryDensity(*hemocell.lattice, outlet, 1.0);
    if (number("twice", 0)) boundary->addVelocityBoundary0N(outlet, *hemocell.lattice);
    delete boundary;
  }

  if (opt.count("checkpoint") && opt["checkpoint"] == "load") hemocell.loadCheckPoint();
  else if (with_cells) hemocell.loadParticles();

  for (plint i = 0; i < (*cfg)["parameters"]["warmup"].read<plint>(); ++i) hemocell.lattice->collideAndStream();

  pcout << "(PipePreInlet) Starting simulation..." << endl;
  const long timing = number("timing", -1);
  std::chrono::steady_clock::time_point t0;
  while (hemocell.iter < tmax) {
    if ((long)hemocell.iter == timing) { hemocell.flush(); hc_synchronize(); t0 = std::chrono::steady_clock::now(); }
    hemocell.iterate();
    if (hemocell.partOfpreInlet) hemocell.preInlet->setDrivingForce();   // never taken on this back end: iterate() does it
    hemocell.preInlet->applyPreInlet();
    if (do_dump && (hemocell.iter == 1 || hemocell.iter == tmax)) dump(hemocell);
  }

  if (timing >= 0 && (long)tmax > timing) {
    hemocell.flush(); hc_synchronize();
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    pcout << "(PipePreInlet) wall time per iteration " << us / (double)(tmax - timing) << " us over " << tmax - timing << " iterations" << endl;
  }
  long counts[4]; hemocell.preInlet->cellCounts(counts);
  hlog << "(PipePreInlet) cells injected " << counts[0] << " rejected " << counts[1] << " removed by the sink " << counts[2] << " checks " << counts[3] << endl;
  if (with_cells) {
    hlog << "(PipePreInlet) # of cells: " << CellInformationFunctionals::getTotalNumberOfCells(&hemocell)
         << " | # of RBC: " << CellInformationFunctionals::getNumberOfCellsFromType(&hemocell, "RBC")
         << ", PLT: " << CellInformationFunctionals::getNumberOfCellsFromType(&hemocell, "PLT") << endl;
  }
  FluidStatistics finfo = FluidInfo::calculateVelocityStatistics(&hemocell);
  hlog << "(PipePreInlet) velocity max " << finfo.max << " mean " << finfo.avg << " lu" << endl;
  if (number("output", 0)) hemocell.writeOutput();
  if (opt.count("checkpoint") && opt["checkpoint"] == "save") { hemocell.saveCheckPoint(); hemocell.saveCheckPoint(); }
  pcout << "(PipePreInlet) DONE iteration " << hemocell.iter << endl;
  return 0;
}
