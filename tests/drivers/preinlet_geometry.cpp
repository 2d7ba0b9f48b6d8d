// The pre-inlet's host-side geometry and pulse functions (hemocell_amd/compat/preInlet.h) on hand-made inputs; no device.
//   preinlet_geometry geometry <direction> <slice|auto|thick|empty> <lengthN> <envelope> <clip 0|1>
//     a 9 x 7 x 7 flag matrix, fluid where the two in-plane coordinates (ascending axis order) lie in [2, 4] x [4, 6]
//   preinlet_geometry interpolate <x> <extrapolate 0|1>      on the five-point table below
//   preinlet_geometry pulse <pFrequency> <t>
//   preinlet_geometry refuse <twice|outside|le-then-open|open-then-le>      the Zou-He names' refusals on a 6 x 5 x 5 lattice
#define HEMOCELL_COMPAT_MAIN
#include "preInlet.h"
#include "helper/leesEdwardsBC.h"

#include <cstring>

int main(int argc, char *argv[]) {
  const std::vector<double> times = {0.0, 0.25, 0.5, 0.75, 1.0}, values = {0.6, 1.4, 1.0, 0.7, 0.6};
  if (argc >= 4 && !std::strcmp(argv[1], "interpolate")) {
    std::printf("%.17g\n", hemo::preInletInterpolate(times, values, std::atof(argv[2]), std::atoi(argv[3]) != 0));
    return 0;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "pulse")) {
    double avg = 0; for (double v : values) avg += v; avg /= (double)values.size();
    std::printf("%.17g\n", hemo::preInletPulseFactor(times, values, avg, std::atof(argv[2]), times.back(), std::atof(argv[3])));
    return 0;
  }
  if (argc >= 3 && !std::strcmp(argv[1], "refuse")) {
    plb::MultiBlockLattice3D<T, DESCRIPTOR> lattice(plb::defaultMultiBlockPolicy3D().getMultiBlockManagement(6, 5, 5), nullptr, nullptr, nullptr,
                                                    new plb::GuoExternalForceBGKdynamics<T, DESCRIPTOR>(1.0));
    plb::OnLatticeBoundaryCondition3D<T, DESCRIPTOR> *bc = plb::createZouHeBoundaryCondition3D<T, DESCRIPTOR>();
    double *displacement = nullptr;
    const std::string what = argv[2];
    if (what == "le-then-open") { hemo::LeesEdwardsBC<T, DESCRIPTOR> le(lattice, 1e-4, 1e-7, &displacement); le.initialize(); }
    bc->addVelocityBoundary0N(plb::Box3D(0, 0, 0, 4, 0, 4), lattice);
    bc->addPressureBoundary0P(plb::Box3D(5, 5, 0, 4, 0, 4), lattice, plb::boundary::density);
    setBoundaryVelocity(lattice, plb::Box3D(0, 0, 1, 3, 1, 3), plb::Array<T, 3>(0.01, 0., 0.));
    setBoundaryDensity(lattice, plb::Box3D(5, 5, 0, 4, 0, 4), 1.01);
    std::printf("declared %zu records, %zu + %zu nodes, u %.17g rho %.17g mask %d\n", lattice.open_decls.size(), lattice.open_decls[0].values.size(),
                lattice.open_decls[1].values.size(), lattice.open_decls[0].values[6][0], lattice.open_decls[1].values[0][3], (int)lattice.mask[6]);
    std::fflush(stdout);
    if (what == "twice") bc->addPressureBoundary1N(plb::Box3D(0, 5, 0, 0, 2, 2), lattice);
    if (what == "outside") bc->addVelocityBoundary2P(plb::Box3D(2, 2, 2, 2, 5, 5), lattice);
    if (what == "open-then-le") { hemo::LeesEdwardsBC<T, DESCRIPTOR> le(lattice, 1e-4, 1e-7, &displacement); le.initialize(); }
    std::printf("not refused\n");
    return 0;
  }
  if (argc < 7 || std::strcmp(argv[1], "geometry")) return 2;
  const char *names[6] = {"Xpos", "Xneg", "Ypos", "Yneg", "Zpos", "Zneg"};
  int d = -1; for (int i = 0; i < 6; i++) if (!std::strcmp(argv[2], names[i])) d = i;
  if (d < 0) return 2;
  const Direction direction = (Direction)d;
  int axis, sign; hemo::direction_axis(direction, axis, sign);
  const std::string mode = argv[3];
  plb::MultiScalarField3D<int> flags(9, 7, 7, 0);
  if (mode != "empty")
    for (plint x = 0; x < 9; x++) for (plint y = 0; y < 7; y++) for (plint z = 0; z < 7; z++) {
      const plint u = axis == 0 ? y : x, v = axis == 2 ? y : z;
      flags.get(x, y, z) = (u >= 2 && u <= 4 && v >= 4 && v <= 6) ? 1 : 0;
    }
  const plb::Box3D system = flags.getBoundingBox();
  plb::Box3D slice = system;
  if (sign < 0) hemo::box_hi(slice, axis) = hemo::box_lo(slice, axis) + (mode == "thick" ? 1 : 0);
  else hemo::box_lo(slice, axis) = hemo::box_hi(slice, axis) - (mode == "thick" ? 1 : 0);
  const plint lengthN = std::atol(argv[4]), envelope = std::atol(argv[5]);
  const plb::Box3D *sys = std::atoi(argv[6]) ? &system : nullptr;
  const hemo::PreInletGeometry g = mode == "auto" ? hemo::autoPreInletGeometry(flags, direction, lengthN, envelope, sys)
                                                   : hemo::preInletGeometry(flags, direction, slice, lengthN, envelope, sys);
  if (!g.error.empty()) { std::printf("refused: %s\n", g.error.c_str()); return 1; }
  auto box = [](const char *name, const plb::Box3D &b) { std::printf("%s %ld %ld %ld %ld %ld %ld\n", name, b.x0, b.x1, b.y0, b.y1, b.z0, b.z1); };
  box("location", g.location); box("fluidInlet", g.fluidInlet); box("sendBox", g.sendBox);
  std::printf("offset %ld %ld %ld\n", g.offset.x, g.offset.y, g.offset.z);
  double window[2], shift[3]; hemo::preInletInjection(g, window, shift);
  std::printf("window %.17g %.17g\nshift %.17g %.17g %.17g\n", window[0], window[1], shift[0], shift[1], shift[2]);
  return 0;
}
