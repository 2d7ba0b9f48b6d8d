// hemo::LeesEdwardsBC (helper/leesEdwardsBC.h of the reference): unbounded simple shear along x between the two z faces of
// an all-periodic lattice.  The reference integrates two data processors into the lattice; here the pass is part of the
// library's step (hcl_set_lees_edwards), and this class only hands the lattice its velocities and displacement.
#pragma once
#include "../hemocell.h"

namespace hemo {

template <typename T, template <class U> class Descriptor>
class LeesEdwardsBC {
 public:
  plb::MultiBlockLattice3D<T, Descriptor> &lattice;
  plint nx, ny, nz;
  double LEdisplacement;                 // displacement per time step
  static double LEcurrentDisplacement;   // current total displacement
  T dt;
  T topVelocity, bottomVelocity;         // macroscopic velocity of the top / bottom layer
  plint dataProcessorLevel;              // the level the reference integrates its processors at (recorded, not used)

  LeesEdwardsBC(plb::MultiBlockLattice3D<T, Descriptor> &lattice_, T shearRate, T dt_, double **hemoCellLEcurrentDisplacement, plint dataProcessorLevel_ = 1)
      : lattice(lattice_) {
    nx = lattice.getNx(); ny = lattice.getNy(); nz = lattice.getNz();
    dt = dt_;
    LEdisplacement = shearRate * dt;
    T vHalf = (nz - 1) * shearRate * 0.5;
    topVelocity = -vHalf;
    bottomVelocity = vHalf;
    dataProcessorLevel = dataProcessorLevel_;
    *hemoCellLEcurrentDisplacement = &LEcurrentDisplacement;   // HemoCell::LEcurrentDisplacement points at this value
  }

  // all three axes periodic, and the pass on from the next step on (and in lattice->initialize())
  void initialize() {
    if (!lattice.open_decls.empty()) lattice.refuse_open("a Lees-Edwards boundary on a lattice with open boundaries: the two do not combine");
    lattice.periodicity().toggleAll(true);
    if (lattice.before_access) lattice.before_access();
    lattice.le.on = true;
    lattice.le.v_top = topVelocity; lattice.le.v_bottom = bottomVelocity;
    lattice.le.d = LEdisplacement;
    lattice.le.cur = &LEcurrentDisplacement;
    lattice.dirty_layout = true;   // the device lattice is (re)created with the boundary
  }

  void updateLECurDisplacement(unsigned int iter) { LEcurrentDisplacement = std::fmod(LEdisplacement * iter, (double)nx); }
};

template <typename T, template <typename U> class Descriptor>
double LeesEdwardsBC<T, Descriptor>::LEcurrentDisplacement = 0;

}  // namespace hemo
