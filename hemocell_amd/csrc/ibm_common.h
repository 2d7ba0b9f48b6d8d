// The device pieces under the immersed-boundary kernels of ibm.hip: the node velocity behind every interpolation, the geometry
// of a per-cell tile, the compaction of the nodes a cell touches, and the one compile-time description of a stencil width
// (Phi<W>: two, three or four points per axis) over which every kernel there is written once.  Everything is kept in an
// unnamed namespace; include it from ibm.hip only.
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

// local (wrapped) origin and decode reciprocals; false when the tile cannot be used (cap: the tile nodes the kernel has LDS for)
__device__ __forceinline__ bool tile_finish(const LatView &v, Tile &t, int cap) {
  if (t.vol > cap) return false;
  if ((v.wrap_x && t.e[0] > v.nx) || (v.per_y && t.e[1] > v.ny) || (v.per_z && t.e[2] > v.nz)) return false;
  t.ow[0] = v.wrap_x ? (int)pmod((long)t.o[0] - v.x0, v.nx) : t.o[0] - v.x0;
  t.ow[1] = v.per_y ? (int)pmod(t.o[1], v.ny) : t.o[1];
  t.ow[2] = v.per_z ? (int)pmod(t.o[2], v.nz) : t.o[2];
  t.r1 = 1.0f / (float)t.e[1]; t.r2 = 1.0f / (float)t.e[2];
  return true;
}

// Is every node of the tile an ordinary fluid node inside the domain?  Then interpolationCoefficientsPhi2 admits every node
// with a non-zero weight and the mask need not be looked at (most cells of a vessel are nowhere near its wall).  Answered
// from one byte per 8 x 8 x 8 brick of the padded lattice (hc_lattice::wallbrick: set when the brick holds a non-fluid node or
// touches a face the stencils cannot cross); a tile covers at most 4 x 4 x 4 bricks, one per lane of wave 0.
__device__ __forceinline__ bool tile_is_clear(const LatView &v, const Tile &t) {
  __shared__ int s_near;
  const int n[3] = {v.nx, v.ny, v.nz};
  bool inside = v.wallbrick != nullptr;
  int b0[3], nb[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int lo = a == 0 ? t.ow[0] + HALO : t.ow[a], hi = lo + t.e[a] - 1, lim = a == 0 ? v.nx + 2 * HALO : n[a];   // x in padded planes
    inside = inside && lo >= 0 && hi < lim && (a != 0 || !v.wrap_x || (t.ow[0] >= 0 && t.ow[0] + t.e[0] <= v.nx));
    b0[a] = lo >> 3; nb[a] = (hi >> 3) - b0[a] + 1;
  }
  if (!inside) return false;   // uniform: the tile wraps around a periodic face or leaves the addressable range
  if (nb[0] * nb[1] * nb[2] > 64) return false;   // uniform: a thin, long tile (5832 nodes can span more bricks than one wave looks at) takes the mask path
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    bool near = false;
    if (l < nb[0] * nb[1] * nb[2]) {
      const int bz = l % nb[2], by = (l / nb[2]) % nb[1], bx = l / (nb[2] * nb[1]);
      near = v.wallbrick[((long)(b0[0] + bx) * v.nby + (b0[1] + by)) * v.nbz + (b0[2] + bz)] != 0;
    }
    const unsigned long long any = __ballot(near);
    if (l == 0) s_near = any != 0ull;
  }
  __syncthreads();
  return s_near == 0;
}

// ----------------------------------------------------------------------------
// Phi<W>: what differs between the delta functions of two, three and four points per axis.  Everything around them is
// interpolationCoefficientsPhi2 (core/immersedBoundaryMethod.h:99-137) as cells.h phi2_stencil states it: the weight of a node
// is phi(dx) * phi(dy) * phi(dz), the W x W x W nodes are visited in ascending x, then y, then z, a node beyond a non-periodic
// face, a node that is not fluid and a zero weight are skipped, and the admitted weights are multiplied by 1 / total.  The
// reference declares phi3, phi4 and their interpolationCoefficients (:43-50, :140-153) and implements none of them; the
// definitions below are this back end's own (include/hemocell_amd.h).
//
// A policy states:
//   TILE, NODES      caps of the per-cell kernels: tile nodes and distinct touched nodes they have LDS for
//   WALL_BRICKS      whether a cell kernel may skip the mask tile where tile_is_clear says so
//   Kept             what a thread keeps of a vertex across the passes of a per-cell kernel
//   rows             lowest stencil node per axis (global coordinates: identical bits wherever the vertex is looked at), and
//                    what of Kept can be formed before the tile is known
//   admit            admission against the LDS copy of the mask (mt; null: no wall anywhere near the cell)
//   for_each(kept)   f(tile index, weight) for every admitted node, in the reference's order
//   Global, Axes,    admission against the lattice's mask: the per-vertex forms, and the cells that do not fit a tile
//   stencil, none    ... and the stencil that admits nothing
//   for_each(global) f(k, admitted, node, lx, ly, lz, weight) for all W^3 nodes in the reference's order, k counting them (the
//                    entries of the reproducible spread keep the place of a node that is not admitted)
//
// Caps.  All two-point stencils of a 642-vertex RBC (radius 7.82 lu) fall into 18 nodes along an axis, so 19 with three points
// (c - 1 .. c + 1 around the two-point pair) and 20 with four (f - 1 .. f + 2).  Node caps: distinct stencil nodes of the
// RBC_FROM_SPHERE mesh at 2000 random orientations and offsets, every second one stretched by 10 % along an axis, counted on the
// CPU: at most 1432 (two points), 2234 (three), 3015 (four); the largest box was 5508 and 6498 nodes.
// LDS per workgroup = 2 * TILE (slots) + max(TILE, 2 * NODES) (mask tile / node list) + 24 * NODES (three doubles per node) +
// 104: 53.2 KiB at W = 2, three workgroups in the 160 KiB of a CU; 77.2 KiB at W = 3, two; 107.5 KiB at W = 4, one.
constexpr int TILE_CAP = 5832;       // 18 x 18 x 18, any orientation of a 642-vertex RBC
constexpr int NODE_CAP = 1536;       // an RBC touches ~1300
constexpr int TILE_CAP3 = 6859;      // 19 x 19 x 19
constexpr int NODE_CAP3 = 2432;
constexpr int TILE_CAP4 = 8000;      // 20 x 20 x 20
constexpr int NODE_CAP4 = 3584;
constexpr int NVPT = 3;        // vertices per thread held in registers (642 vertices / 256 threads)
// Four waves per workgroup (MAXW).  Eight waves per cell (512 threads, two vertices each) were tried for both two-point kernels: the spread gains 3.5 % at 10 % hematocrit
// and nothing at 25 % (and loses once its loads are reordered), the interpolation loses 9-15 % (184 VGPRs: one cell per CU);
// capping the interpolation at 168 / 128 VGPRs for three cells per CU spills and loses 15 %.  Both kernels wait 80 % of their
// wave cycles (rocprofv3 SQ_WAIT_ANY + SQ_WAIT_INST_ANY) and respond to neither more waves nor shorter workgroups.

template <int N> struct Phi;

// Two points keep the 8 normalised products: base = tile index of the lowest corner; adm = admitted-node bits (bit 4 i + 2 j + k)
struct VStencil { double w[8]; int base; unsigned adm; };

template <> struct Phi<2> {
  static constexpr int W = 2, TILE = TILE_CAP, NODES = NODE_CAP;
  static constexpr bool WALL_BRICKS = true;
  using Kept = VStencil;
  using Global = Stencil;
  struct Axes {};
  // nearest node, minus one when the vertex lies below it; the products wait for the mask tile
  static __device__ __forceinline__ void rows(const double p[3], int b[3], Kept &) {
#pragma unroll
    for (int a = 0; a < 3; a++) { const long c = nearest_node(p[a]); b[a] = (int)c + ((p[a] < (double)c) ? -1 : 0); }
  }
  // same arithmetic and visiting order as phi2_stencil
  static __device__ __forceinline__ void admit(const Tile &t, const unsigned char *mt, const double p[3], const int b[3], Kept &o) {
    const int sy = t.e[2], sx = t.e[1] * t.e[2];
    o.base = ((b[0] - t.o[0]) * t.e[1] + (b[1] - t.o[1])) * t.e[2] + (b[2] - t.o[2]);
    o.adm = 0;
    double total = 0.0;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
          const int idx = i * 4 + j * 2 + k;
          const double weight = phi2(p[0] - (double)(b[0] + i)) * phi2(p[1] - (double)(b[1] + j)) * phi2(p[2] - (double)(b[2] + k));
          const bool adm = (weight != 0.0) && (!mt || mt[o.base + i * sx + j * sy + k] == 0);
          if (adm) { total += weight; o.adm |= 1u << idx; }
          o.w[idx] = adm ? weight : 0.0;
        }
    const double coeff = 1.0 / total;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) o.w[idx] *= coeff;
  }
  template <class F> static __device__ __forceinline__ void for_each(const Kept &s, int sx, int sy, F f) {
#pragma unroll
    for (int k = 0; k < 8; k++) if (s.adm & (1u << k)) f(s.base + (k >> 2) * sx + ((k >> 1) & 1) * sy + (k & 1), s.w[k]);
  }
  static __device__ __forceinline__ void stencil(const LatView &v, double px, double py, double pz, Global &g, Axes &) { phi2_stencil(v, px, py, pz, g); }
  static __device__ __forceinline__ void none(Global &g) {
#pragma unroll
    for (int k = 0; k < 8; k++) { g.node[k] = -1; g.w[k] = 0.0; g.lx[k] = g.ly[k] = g.lz[k] = 0; }
  }
  template <class F> static __device__ __forceinline__ void for_each(const LatView &, const Global &g, const Axes &, F f) {
#pragma unroll
    for (int k = 0; k < 8; k++) f(k, g.node[k] >= 0, g.node[k], g.lx[k], g.ly[k], g.lz[k], g.w[k]);
  }
};

__device__ __forceinline__ double phi3(double r) {
  r = fabs(r);
  if (r <= 0.5) return (1.0 + sqrt(1.0 - 3.0 * r * r)) / 3.0;
  if (r <= 1.5) return (5.0 - 3.0 * r - sqrt(-2.0 + 6.0 * r - 3.0 * r * r)) / 6.0;
  return 0.0;
}
__device__ __forceinline__ double phi4(double r) {
  r = fabs(r);
  if (r <= 1.0) return (3.0 - 2.0 * r + sqrt(1.0 + 4.0 * r - 4.0 * r * r)) / 8.0;
  if (r <= 2.0) return (5.0 - 2.0 * r - sqrt(-7.0 + 12.0 * r - 4.0 * r * r)) / 8.0;
  return 0.0;
}

// Three and four points keep the three per-axis weight rows, the bits of the admitted nodes (bit (i W + j) W + k) and the
// normaliser -- never the W^3 products (81 or 192 doubles for three vertices would not stay in registers); a weight is formed
// where it is used.  base: tile index of the lowest node of the stencil.
template <int W> struct WStencil { double wx[W], wy[W], wz[W]; double coeff; unsigned long long adm; int base; };

template <int N> struct Phi {
  static constexpr int W = N, TILE = N == 3 ? TILE_CAP3 : TILE_CAP4, NODES = N == 3 ? NODE_CAP3 : NODE_CAP4;
  // the mask tile is always filled: with 27 or 64 nodes per vertex its bytes are a small part of the work, and the shortcut
  // would have to prove a box of 20^3 clear
  static constexpr bool WALL_BRICKS = false;
  using Kept = WStencil<W>;
  using Global = Kept;   // base unused
  // per-axis local (wrapped) coordinates of the W rows of a stencil, and which of them can be addressed: the rules of phi2_stencil.
  // An object of its own: the four-point per-vertex interpolation indexes both at run time, and the compiler finds LDS for this
  // one only while it is apart from the rows
  struct Axes { int l[3][W]; bool ok[3][W]; };

  static __device__ __forceinline__ double phi(double r) { if constexpr (W == 3) return phi3(r); else return phi4(r); }
  static __device__ __forceinline__ double weight(const Kept &s, int i, int j, int k) { return s.wx[i] * s.wy[j] * s.wz[k]; }
  static __device__ __forceinline__ long node(const LatView &v, const Axes &ax, int i, int j, int k) {
    return (long)(ax.l[0][i] + HALO) * v.plane + (long)ax.l[1][j] * v.nz + ax.l[2][k];
  }

  // three points: nearest node - 1; four points: floor - 1
  static __device__ __forceinline__ void rows(const double p[3], int b[3], Kept &s) {
#pragma unroll
    for (int a = 0; a < 3; a++) b[a] = (int)(W == 3 ? nearest_node(p[a]) : (long)floor(p[a])) - 1;
#pragma unroll
    for (int i = 0; i < W; i++) { s.wx[i] = phi(p[0] - (double)(b[0] + i)); s.wy[i] = phi(p[1] - (double)(b[1] + i)); s.wz[i] = phi(p[2] - (double)(b[2] + i)); }
  }
  static __device__ __forceinline__ void admit(const Tile &t, const unsigned char *mt, const double *, const int b[3], Kept &s) {
    const int sy = t.e[2], sx = t.e[1] * t.e[2];
    s.base = ((b[0] - t.o[0]) * t.e[1] + (b[1] - t.o[1])) * t.e[2] + (b[2] - t.o[2]);
    s.adm = 0;
    double total = 0.0;
#pragma unroll
    for (int i = 0; i < W; i++)
#pragma unroll
      for (int j = 0; j < W; j++)
#pragma unroll
        for (int k = 0; k < W; k++) {
          const double wt = weight(s, i, j, k);
          if (wt != 0.0 && mt[s.base + i * sx + j * sy + k] == 0) { total += wt; s.adm |= 1ull << ((i * W + j) * W + k); }
        }
    s.coeff = 1.0 / total;
  }
  template <class F> static __device__ __forceinline__ void for_each(const Kept &s, int sx, int sy, F f) {
    if (!s.adm) return;
#pragma unroll
    for (int i = 0; i < W; i++)
#pragma unroll
      for (int j = 0; j < W; j++)
#pragma unroll
        for (int k = 0; k < W; k++)
          if (s.adm & (1ull << ((i * W + j) * W + k))) f(s.base + i * sx + j * sy + k, weight(s, i, j, k) * s.coeff);
  }
  static __device__ __forceinline__ void stencil(const LatView &v, double px, double py, double pz, Global &s, Axes &ax) {
    const double p[3] = {px, py, pz};
    int b[3];
    rows(p, b, s);
#pragma unroll
    for (int i = 0; i < W; i++) {
      const long gx = (long)b[0] + i, gy = (long)b[1] + i, gz = (long)b[2] + i;
      long lx = gx - v.x0, ly = gy, lz = gz;
      bool okx = true, oky = true, okz = true;
      if (v.wrap_x) lx = pmod(lx, v.nx);
      else if (v.halo_x) okx = lx >= -HALO && lx < v.nx + HALO;
      else okx = lx >= 0 && lx < v.nx;
      if (gy < 0 || gy >= v.ny) { if (v.per_y) ly = pmod(gy, v.ny); else oky = false; }
      if (gz < 0 || gz >= v.nz) { if (v.per_z) lz = pmod(gz, v.nz); else okz = false; }
      ax.l[0][i] = (int)lx; ax.l[1][i] = (int)ly; ax.l[2][i] = (int)lz;
      ax.ok[0][i] = okx; ax.ok[1][i] = oky; ax.ok[2][i] = okz;
    }
    s.base = 0; s.adm = 0;
    double total = 0.0;
#pragma unroll
    for (int i = 0; i < W; i++)
#pragma unroll
      for (int j = 0; j < W; j++)
#pragma unroll
        for (int k = 0; k < W; k++) {
          const double wt = weight(s, i, j, k);
          bool adm = ax.ok[0][i] && ax.ok[1][j] && ax.ok[2][k] && wt != 0.0;
          if (adm) adm = v.mask[node(v, ax, i, j, k)] == 0;
          if (adm) { total += wt; s.adm |= 1ull << ((i * W + j) * W + k); }
        }
    s.coeff = 1.0 / total;
  }
  static __device__ __forceinline__ void none(Global &s) { s.base = 0; s.adm = 0; s.coeff = 0.0; }
  template <class F> static __device__ __forceinline__ void for_each(const LatView &v, const Global &s, const Axes &ax, F f) {
#pragma unroll
    for (int i = 0; i < W; i++)
#pragma unroll
      for (int j = 0; j < W; j++)
#pragma unroll
        for (int k = 0; k < W; k++) {
          const int n = (i * W + j) * W + k;
          if (s.adm & (1ull << n)) f(n, true, node(v, ax, i, j, k), ax.l[0][i], ax.l[1][j], ax.l[2][k], weight(s, i, j, k) * s.coeff);
          else f(n, false, -1L, 0, 0, 0, 0.0);
        }
  }
};

// Compacts the nodes the cell's stencils admit: slot[tile index] = rank of the node, list[rank] = tile index, in tile order within
// each wave's 256 tile entries (runs along z stay runs).  One LDS atomic per wave, ranks within the wave from its ballot.  Returns
// the node count (uniform); a count above S::NODES means the list is incomplete and the caller takes its fallback path.
constexpr unsigned short SLOT_FREE = 0xFFFF, SLOT_MARK = 0xFFFE;
template <class S>
__device__ __forceinline__ int compact_nodes(const Tile &t, const typename S::Kept vs[NVPT], unsigned short *slot, unsigned short *list, int *s_count) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
  for (int i = tid; i < t.vol; i += nth) slot[i] = SLOT_FREE;
  if (tid == 0) *s_count = 0;
  __syncthreads();   // also: every thread is done reading the mask tile, list may overwrite it
#pragma unroll
  for (int j = 0; j < NVPT; j++) S::for_each(vs[j], sx, sy, [&](int at, double) __attribute__((always_inline)) { slot[at] = SLOT_MARK; });
  __syncthreads();
  for (int i0 = 0; i0 < t.vol; i0 += nth) {
    const int i = i0 + tid;
    const bool marked = i < t.vol && slot[i] == SLOT_MARK;
    const unsigned long long b = __ballot(marked);
    int first = 0;
    if ((tid & 63) == 0 && b) first = atomicAdd(s_count, (int)__popcll(b));
    first = __shfl(first, 0);
    if (marked) {
      const int n = first + (int)__popcll(b & ((1ull << (tid & 63)) - 1ull));
      if (n < S::NODES) { slot[i] = (unsigned short)n; list[n] = (unsigned short)i; }
    }
  }
  __syncthreads();
  return *s_count;
}

}  // namespace

// K<OPEN> through the one open-boundary dispatch (hc::launch_open)
#define HC_LAUNCH_POPS(K, grid, block, v, pv, ...)                                                                      \
  hc::launch_open(L, pv, [&](auto open, const auto &pops) {                                                             \
    hipLaunchKernelGGL(K<decltype(open)::value>, grid, block, 0, hc::stream(), v, pops, __VA_ARGS__);                   \
  })
