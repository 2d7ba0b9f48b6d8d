// What the two immersed-boundary translation units share (ibm.hip: the two-point kernels, ibm_wide.hip: the three- and
// four-point kernels): the node velocity behind every interpolation, and the geometry of a per-cell tile.  The pieces were
// written for ibm.hip and are kept in an unnamed namespace, as they were there, so that the kernels of ibm.hip keep their
// symbols; include it from those two files only.
#pragma once
#include "cells.h"
#include <type_traits>

namespace {

// ----------------------------------------------------------------------------
// interpolate: v = sum_j w_j * (j/rho + F/2)(node_j) on the post-stream state
struct PopView {
  const double *f; const double *F; double bx, by, bz; long qs;   // qs: population stride
  hc::BodyRegions reg;
};
// lattices with Zou-He open boundaries (hc_lattice::ob_n > 0) run the OPEN instantiations of the interpolation kernels: the
// gathered populations of a fluid open-boundary node are completed (zou_he_node, as the collide is about to) before the moments
// are taken.  Every other lattice keeps PopView, its kernel-argument block and its code.
struct OpenPopView : PopView { const int *ob_code; const double *ob_val; };
template <bool OPEN> using Pops = std::conditional_t<OPEN, OpenPopView, PopView>;

template <bool OPEN = false>
__device__ __forceinline__ void node_velocity(const LatView &v, const Pops<OPEN> &pv, int lx, int ly, int lz, long node, double u[3]) {
  // A node on the OUTER halo plane of a slab would pull from beyond the allocation.  Only particles whose nearest node lies
  // outside the slab have such a node in their stencil, and their interpolated velocity is never used (the owner's record
  // replaces it, "a local particle wins"), so the value does not matter -- the access must not happen.
  if (v.halo_x && (lx <= -HALO || lx >= v.nx + HALO - 1)) { u[0] = u[1] = u[2] = 0.0; return; }
  // first halo plane of a slab: the neighbour that owns the node has evaluated this very expression and sent the result
  // (3 doubles per node instead of the 19 population planes the gather below would need, slab.hip)
  if (v.halo_x && (lx == -1 || lx == v.nx)) {
    const double *hu = v.halo_u[lx < 0 ? 0 : 1];
    if (hu) { const long k = (long)ly * v.nz + lz; u[0] = hu[k]; u[1] = hu[v.ny_nz + k]; u[2] = hu[2L * v.ny_nz + k]; return; }
  }
  // gather S(node,q) = P(node - c_q, q) through the neighbour and wrap rules the collide kernel uses (d3q19.h)
  const hc::Nbr nb = hc::neighbours(v, v.plane, lx, ly, lz);
  double r = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
  [[maybe_unused]] double f[OPEN ? HC_Q : 1];   // OPEN: the gathered populations are kept, completed, and summed afterwards in the same order
#define M(Q, CX, CY, CZ)                                                              \
  {                                                                                   \
    bool ok; const long off = hc::src_off<CX, CY, CZ>(nb, ok);                        \
    const double fq = ok ? pv.f[(long)Q * pv.qs + node + off] : 0.0;                 \
    if constexpr (OPEN) f[Q] = fq;                                                    \
    else {                                                                            \
      r += fq;                                                                        \
      if (CX == 1) jx += fq; else if (CX == -1) jx += -fq;                            \
      if (CY == 1) jy += fq; else if (CY == -1) jy += -fq;                            \
      if (CZ == 1) jz += fq; else if (CZ == -1) jz += -fq;                            \
    }                                                                                 \
  }
  FOR_Q(M)
#undef M
  if constexpr (OPEN) {
    if (v.mask[node] == 0) {
      const int code = pv.ob_code[node];
      if (code >= 0) hc::zou_he_node(f, code, pv.ob_val);
    }
    hc::moments(f, r, jx, jy, jz);
  }
  const double invRho = 1.0 / (1.0 + r);
  double bx = pv.bx, by = pv.by, bz = pv.bz;
  if (pv.reg.n) {   // a halo plane of a slab, or the wrapped image, is the global node next door
    int xg = v.x0 + lx;
    if (xg < 0) xg += v.nx_global; else if (xg >= v.nx_global) xg -= v.nx_global;
    region_force(pv.reg, xg, ly, lz, bx, by, bz);
  }
  u[0] = jx * invRho + (bx + pv.F[3 * node]) / 2.0;
  u[1] = jy * invRho + (by + pv.F[3 * node + 1]) / 2.0;
  u[2] = jz * invRho + (bz + pv.F[3 * node + 2]) / 2.0;
}

// state after hcl_step_end: f[cur] holds the populations just written, force[(fcur+2)%3] the force they were collided with
PopView make_pops(const hc_lattice *L) {
  return PopView{L->f[L->cur], L->force[(L->fcur + 2) % 3], L->body[0], L->body[1], L->body[2], (long)L->qstride, L->regions};
}
// the arguments of the open-boundary instantiations (hc::launch_open)
OpenPopView open_of(const hc_lattice *L, const PopView &pv) {
  OpenPopView o;
  static_cast<PopView &>(o) = pv;
  o.ob_code = L->ob_code; o.ob_val = L->ob_val;
  return o;
}

// ----------------------------------------------------------------------------
// the tile of a per-cell kernel: bounding box of a cell's stencil nodes: origin o (global), extent e, origin ow in local
// wrapped coordinates, reciprocals for the index decode
struct Tile { int o[3]; int e[3]; int vol; int ow[3]; float r1, r2; };

// tile index -> (tx, ty, tz) without integer division.  Exact for i < 2^16: (i + 0.5) / e is at least 0.5 / e
// away from an integer while the float error stays below 1e-3 / e.
__device__ __forceinline__ void tile_decode(const Tile &t, int i, int &tx, int &ty, int &tz) {
  const int q = (int)(((float)i + 0.5f) * t.r2);
  tz = i - q * t.e[2];
  tx = (int)(((float)q + 0.5f) * t.r1);
  ty = q - tx * t.e[1];
}

// global lattice element of tile entry i (only meaningful for entries that were admitted by a stencil)
__device__ __forceinline__ long tile_node(const LatView &v, const Tile &t, int i, int &lx, int &ly, int &lz) {
  int tx, ty, tz;
  tile_decode(t, i, tx, ty, tz);
  lx = t.ow[0] + tx; ly = t.ow[1] + ty; lz = t.ow[2] + tz;
  if (v.wrap_x && lx >= v.nx) lx -= v.nx;     // the tile is no wider than the domain (cell_prologue), one wrap suffices
  if (v.per_y && ly >= v.ny) ly -= v.ny;
  if (v.per_z && lz >= v.nz) lz -= v.nz;
  return (long)(lx + HALO) * v.plane + ly * v.nz + lz;
}

constexpr int MAXW = 4;        // waves per workgroup

// bounding box of all stencil nodes of the cell: per-thread min/max -> wave shuffles -> LDS -> everyone
__device__ __forceinline__ void block_bbox(int lo[3], int hi[3], int *s_red, Tile &t) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], off)); hi[a] = max(hi[a], __shfl_xor(hi[a], off)); }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) { s_red[(tid >> 6) * 6 + a] = lo[a]; s_red[(tid >> 6) * 6 + 3 + a] = hi[a]; }
  }
  __syncthreads();
  const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    int l = s_red[a], h = s_red[3 + a];
    for (int w = 1; w < nw; w++) { l = min(l, s_red[w * 6 + a]); h = max(h, s_red[w * 6 + 3 + a]); }
    t.o[a] = l; t.e[a] = h >= l ? h - l + 1 : 0;   // no live vertex at all (every particle of the cell removed): an empty tile
  }
  const long vol = (long)t.e[0] * t.e[1] * t.e[2];
  t.vol = vol > 0x7fffffff ? 0x7fffffff : (int)vol;
}

// mask class of tile entry i: 0 fluid, 1/2 boundary, 3 not addressable (outside the domain / halo range)
__device__ __forceinline__ unsigned char tile_mask(const LatView &v, const Tile &t, int i) {
  int tx, ty, tz;
  tile_decode(t, i, tx, ty, tz);
  int lx = t.ow[0] + tx, ly = t.ow[1] + ty, lz = t.ow[2] + tz;
  if (v.wrap_x) { if (lx >= v.nx) lx -= v.nx; }
  else if (v.halo_x) { if (lx < -HALO || lx >= v.nx + HALO) return 3; }
  else if (lx < 0 || lx >= v.nx) return 3;
  if (v.per_y) { if (ly >= v.ny) ly -= v.ny; } else if (ly < 0 || ly >= v.ny) return 3;
  if (v.per_z) { if (lz >= v.nz) lz -= v.nz; } else if (lz < 0 || lz >= v.nz) return 3;
  return v.mask[(long)(lx + HALO) * v.plane + ly * v.nz + lz];
}

}  // namespace

// K<OPEN> through the one open-boundary dispatch (hc::launch_open)
#define HC_LAUNCH_POPS(K, grid, block, v, pv, ...)                                                                      \
  hc::launch_open(L, pv, [&](auto open, const auto &pops) {                                                             \
    hipLaunchKernelGGL(K<decltype(open)::value>, grid, block, 0, hc::stream(), v, pops, __VA_ARGS__);                   \
  })
