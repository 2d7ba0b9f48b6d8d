// The one statement of the D3Q19 lattice: the velocity set with its weights, and the neighbour and wrap rules of the gather
// S(node, q) = P(node - c_q, q).  The collide, every observer of lattice.hip and the IBM node velocity of ibm.hip expand this
// table and go through these rules; the host reads the same table as the arrays HC_CX / HC_CY / HC_CZ.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hemocell_amd.h"

// D3Q19, Palabos ordering: opposite of i (1..9) is i+9.   M(q, c_x, c_y, c_z)
// (patch/palabos.patch:491-498)
#define FOR_Q(M)                                                                                     \
  M(0, 0, 0, 0) M(1, -1, 0, 0) M(2, 0, -1, 0) M(3, 0, 0, -1) M(4, -1, -1, 0) M(5, -1, 1, 0)          \
  M(6, -1, 0, -1) M(7, -1, 0, 1) M(8, 0, -1, -1) M(9, 0, -1, 1) M(10, 1, 0, 0) M(11, 0, 1, 0)        \
  M(12, 0, 0, 1) M(13, 1, 1, 0) M(14, 1, -1, 0) M(15, 1, 0, 1) M(16, 1, 0, -1) M(17, 0, 1, 1)        \
  M(18, 0, 1, -1)

namespace hc {

#define M(Q, CX, CY, CZ) CX,
inline constexpr int HC_CX[HC_Q] = {FOR_Q(M)};
#undef M
#define M(Q, CX, CY, CZ) CY,
inline constexpr int HC_CY[HC_Q] = {FOR_Q(M)};
#undef M
#define M(Q, CX, CY, CZ) CZ,
inline constexpr int HC_CZ[HC_Q] = {FOR_Q(M)};
#undef M

__host__ __device__ __forceinline__ constexpr double tq(int q) { return q == 0 ? 1. / 3. : ((q >= 1 && q <= 3) || (q >= 10 && q <= 12)) ? 1. / 18. : 1. / 36.; }

// the table is pinned: entry q sits in slot q, opposite pairs are i and i + 9, and a direction's weight is the one of its
// length, the nineteen of them summing to 1 (counted exactly, in thirty-sixths)
constexpr int q_len2(int q) { return HC_CX[q] * HC_CX[q] + HC_CY[q] * HC_CY[q] + HC_CZ[q] * HC_CZ[q]; }
constexpr bool q_table_ok() {
  int slot = 0, thirty_sixths = 0;
  bool ok = true;
#define M(Q, CX, CY, CZ) ok = ok && Q == slot++;
  FOR_Q(M)
#undef M
  for (int i = 1; i <= 9; i++) ok = ok && HC_CX[i + 9] == -HC_CX[i] && HC_CY[i + 9] == -HC_CY[i] && HC_CZ[i + 9] == -HC_CZ[i];
  for (int q = 0; q < HC_Q; q++) {
    const int n = q_len2(q);
    ok = ok && tq(q) == (n == 0 ? 1. / 3. : n == 1 ? 1. / 18. : 1. / 36.);
    thirty_sixths += n == 0 ? 12 : n == 1 ? 2 : 1;
  }
  return ok && slot == HC_Q && thirty_sixths == 36;
}
static_assert(q_table_ok(), "D3Q19 table");

#ifdef __HIPCC__
struct Nbr {  // element offsets to the -1 / +1 neighbour along each axis, and validity
  long xm, xp;
  int ym, yp, zm, zp;
  bool ym_ok, yp_ok, zm_ok, zp_ok;
};

// a: anything with nx, ny, nz, wrap_x, per_y, per_z (the kernel arguments of lattice.hip, the LatView of the IBM kernels);
// xs: elements from x-plane to x-plane
template <class A>
__device__ __forceinline__ Nbr neighbours(const A &a, long xs, int x, int y, int z) {
  Nbr n;
  n.xm = -xs; n.xp = xs;
  if (a.wrap_x) {
    if (x == 0) n.xm = (long)(a.nx - 1) * xs;
    if (x == a.nx - 1) n.xp = -(long)(a.nx - 1) * xs;
  }
  n.ym = -a.nz; n.yp = a.nz; n.ym_ok = n.yp_ok = true;
  if (y == 0) { if (a.per_y) n.ym = (a.ny - 1) * a.nz; else n.ym_ok = false; }
  if (y == a.ny - 1) { if (a.per_y) n.yp = -(a.ny - 1) * a.nz; else n.yp_ok = false; }
  n.zm = -1; n.zp = 1; n.zm_ok = n.zp_ok = true;
  if (z == 0) { if (a.per_z) n.zm = a.nz - 1; else n.zm_ok = false; }
  if (z == a.nz - 1) { if (a.per_z) n.zp = -(a.nz - 1); else n.zp_ok = false; }
  return n;
}

// offset from a node to (node - c_q)   [c = +1 -> the -1 neighbour]
template <int CX, int CY, int CZ>
__device__ __forceinline__ long src_off(const Nbr &n, bool &ok) {
  long off = 0; ok = true;
  if (CX == 1) off += n.xm; else if (CX == -1) off += n.xp;
  if (CY == 1) { off += n.ym; ok = ok && n.ym_ok; } else if (CY == -1) { off += n.yp; ok = ok && n.yp_ok; }
  if (CZ == 1) { off += n.zm; ok = ok && n.zm_ok; } else if (CZ == -1) { off += n.zp; ok = ok && n.zp_ok; }
  return off;
}
// offset from a node to (node + c_q)
template <int CX, int CY, int CZ>
__device__ __forceinline__ long dst_off(const Nbr &n, bool &ok) {
  long off = 0; ok = true;
  if (CX == 1) off += n.xp; else if (CX == -1) off += n.xm;
  if (CY == 1) { off += n.yp; ok = ok && n.yp_ok; } else if (CY == -1) { off += n.ym; ok = ok && n.ym_ok; }
  if (CZ == 1) { off += n.zp; ok = ok && n.zp_ok; } else if (CZ == -1) { off += n.zm; ok = ok && n.zm_ok; }
  return off;
}

// gather the post-stream populations S(node, q) = P(node - c_q, q)
__device__ __forceinline__ void pull(const double *__restrict__ fin, long npad, long node, const Nbr &n, double f[HC_Q]) {
#define M(Q, CX, CY, CZ)                                   \
  {                                                        \
    bool ok; long off = src_off<CX, CY, CZ>(n, ok);        \
    f[Q] = ok ? fin[(long)Q * npad + node + off] : 0.0;    \
  }
  FOR_Q(M)
#undef M
}

// moments in the oracle's order: ascending q, zero-velocity components skipped
__device__ __forceinline__ void moments(const double f[HC_Q], double &rhoBar, double &jx, double &jy, double &jz) {
  double r = 0.0, x = 0.0, y = 0.0, z = 0.0;
#define M(Q, CX, CY, CZ)              \
  r += f[Q];                          \
  if (CX == 1) x += f[Q]; else if (CX == -1) x += -f[Q]; \
  if (CY == 1) y += f[Q]; else if (CY == -1) y += -f[Q]; \
  if (CZ == 1) z += f[Q]; else if (CZ == -1) z += -f[Q];
  FOR_Q(M)
#undef M
  rhoBar = r; jx = x; jy = y; jz = z;
}

template <int CX, int CY, int CZ>
__device__ __forceinline__ double cdot(double a0, double a1, double a2) {
  // ((cx*a0 + cy*a1) + cz*a2) with the zero terms dropped (exact)
  double s = 0.0; bool first = true;
  if (CX != 0) { s = (CX == 1 ? a0 : -a0); first = false; }
  if (CY != 0) { double t = (CY == 1 ? a1 : -a1); s = first ? t : s + t; first = false; }
  if (CZ != 0) { double t = (CZ == 1 ? a2 : -a2); s = first ? t : s + t; first = false; }
  return s;
}
#endif

}  // namespace hc
