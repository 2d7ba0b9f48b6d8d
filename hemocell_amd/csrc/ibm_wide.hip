// Immersed-boundary coupling with the three-point (Roma) and four-point (Peskin) delta functions: hcp_type_set_ibm_kernel.
//
// The reference declares phi3, phi4, interpolationCoefficientsPhi3 and interpolationCoefficientsPhi4
// (core/immersedBoundaryMethod.h:43-50, :140-153) and implements none of them; the definitions below are this back end's own
// (include/hemocell_amd.h).  Everything around them is interpolationCoefficientsPhi2 (:99-137) as
// cells.h phi2_stencil states it: the weight of a node is phi(dx) * phi(dy) * phi(dz), the W x W x W nodes are visited in
// ascending x, then y, then z, a node beyond a non-periodic face, a node that is not fluid and a zero weight are skipped, and
// the admitted weights are multiplied by 1 / total.  The force limit, the spread and the interpolation sums are those of ibm.hip.
//
// The same three forms as for two points: one thread per vertex (hc_debug_ibm_per_vertex), one workgroup per cell on an LDS
// tile (the default), and the entries of the reproducible spread (hc_set_reproducible_spread).  The kernels of ibm.hip are not
// touched: a type on HC_IBM_PHI2 never comes here.
#include "ibm_common.h"

namespace {

// Caps of the per-cell kernels, one set per width.  A 642-vertex RBC (radius 7.82 lu) reaches at most 18 nodes along an axis
// with two points, so 19 with three (c - 1 .. c + 1 around the two-point pair) and 20 with four (f - 1 .. f + 2).
// Node caps: distinct stencil nodes of the RBC_FROM_SPHERE mesh at 2000 random orientations and offsets, every second one
// stretched by 10 % along an axis, counted on the CPU: at most 1432 (two points), 2234 (three), 3015 (four); the largest box
// was 5508 and 6498 nodes.
// LDS per workgroup = 2 * TILE_CAP (slots) + max(TILE_CAP, 2 * NODE_CAP) (mask tile / node list) + 24 * NODE_CAP (three
// doubles per node) + 104: 77.2 KiB at W = 3, two workgroups in the 160 KiB of a CU; 107.5 KiB at W = 4, one workgroup per CU.
constexpr int TILE_CAP3 = 6859;      // 19 x 19 x 19
constexpr int NODE_CAP3 = 2432;
constexpr int TILE_CAP4 = 8000;      // 20 x 20 x 20
constexpr int NODE_CAP4 = 3584;
template <int W> constexpr int tile_cap() { return W == 3 ? TILE_CAP3 : TILE_CAP4; }
template <int W> constexpr int node_cap() { return W == 3 ? NODE_CAP3 : NODE_CAP4; }
constexpr int NVPT = 3;              // vertices per thread held in registers, as in ibm.hip

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

// What a thread keeps of one vertex: the three per-axis weight rows, the bits of the admitted nodes (bit (i W + j) W + k) and
// the normaliser -- never the W^3 products (81 or 192 doubles for three vertices would not stay in registers).
// base: lowest node of the stencil (global) in the per-vertex forms; tile index of that node in the per-cell kernels.
template <int W> struct WStencil { double wx[W], wy[W], wz[W]; double coeff; unsigned long long adm; int base; };

// rows of one vertex; b: the lowest node per axis (global coordinates: identical bits wherever the vertex is looked at)
template <int W>
__device__ __forceinline__ void wide_rows(double px, double py, double pz, int b[3], WStencil<W> &s) {
  const double p[3] = {px, py, pz};
#pragma unroll
  for (int a = 0; a < 3; a++) b[a] = (int)(W == 3 ? nearest_node(p[a]) : (long)floor(p[a])) - 1;
#pragma unroll
  for (int i = 0; i < W; i++) {
    if constexpr (W == 3) { s.wx[i] = phi3(p[0] - (double)(b[0] + i)); s.wy[i] = phi3(p[1] - (double)(b[1] + i)); s.wz[i] = phi3(p[2] - (double)(b[2] + i)); }
    else { s.wx[i] = phi4(p[0] - (double)(b[0] + i)); s.wy[i] = phi4(p[1] - (double)(b[1] + i)); s.wz[i] = phi4(p[2] - (double)(b[2] + i)); }
  }
}
template <int W> __device__ __forceinline__ double wide_weight(const WStencil<W> &s, int i, int j, int k) { return s.wx[i] * s.wy[j] * s.wz[k]; }

// per-axis local (wrapped) coordinates of the W rows of a stencil, and which of them can be addressed: the rules of phi2_stencil
template <int W> struct WAxes { int l[3][W]; bool ok[3][W]; };
template <int W>
__device__ __forceinline__ void wide_axes(const LatView &v, const int b[3], WAxes<W> &ax) {
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
}
template <int W> __device__ __forceinline__ long wide_node(const LatView &v, const WAxes<W> &ax, int i, int j, int k) {
  return (long)(ax.l[0][i] + HALO) * v.plane + (long)ax.l[1][j] * v.nz + ax.l[2][k];
}

// admission against the lattice's mask (per-vertex forms, and the cells that do not fit a tile)
template <int W>
__device__ __forceinline__ void wide_stencil(const LatView &v, double px, double py, double pz, WStencil<W> &s, WAxes<W> &ax) {
  int b[3];
  wide_rows<W>(px, py, pz, b, s);
  wide_axes<W>(v, b, ax);
  s.base = 0; s.adm = 0;
  double total = 0.0;
#pragma unroll
  for (int i = 0; i < W; i++)
#pragma unroll
    for (int j = 0; j < W; j++)
#pragma unroll
      for (int k = 0; k < W; k++) {
        const double weight = wide_weight<W>(s, i, j, k);
        bool adm = ax.ok[0][i] && ax.ok[1][j] && ax.ok[2][k] && weight != 0.0;
        if (adm) adm = v.mask[wide_node<W>(v, ax, i, j, k)] == 0;
        if (adm) { total += weight; s.adm |= 1ull << ((i * W + j) * W + k); }
      }
  s.coeff = 1.0 / total;
}

// ----------------------------------------------------------------------------
// one thread per vertex
template <int W>
__global__ __launch_bounds__(256) void ibm_wide_spread_kernel(LatView v, long n, const double *px, const double *py, const double *pz,
                                                              double *fx, double *fy, double *fz, const double *rx, const double *ry, const double *rz,
                                                              double *F, int limit_on, double f_limit, const int *vert_cell, const int *tag, const unsigned char *dead) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag[vert_cell[i]] == 1) return;   // removed particle / cell gone
  double f0 = fx[i], f1 = fy[i], f2 = fz[i];
  if (limit_on) {  // FORCE_LIMIT cap, core/hemoCellParticleField.cpp:848-852 (mutates sv.force)
    const double mag = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
    if (mag > f_limit) {
      const double sc = f_limit / mag;
      f0 *= sc; f1 *= sc; f2 *= sc;
      fx[i] = f0; fy[i] = f1; fz[i] = f2;
    }
  }
  const double g0 = (rx ? rx[i] : 0.0) + f0, g1 = (ry ? ry[i] : 0.0) + f1, g2 = (rz ? rz[i] : 0.0) + f2;   // force_repulsion + force, :857-859
  WStencil<W> s; WAxes<W> ax;
  wide_stencil<W>(v, px[i], py[i], pz[i], s, ax);
#pragma unroll
  for (int a = 0; a < W; a++)
#pragma unroll
    for (int b = 0; b < W; b++)
#pragma unroll
      for (int c = 0; c < W; c++) {
        if (!(s.adm & (1ull << ((a * W + b) * W + c)))) continue;
        const long node = wide_node<W>(v, ax, a, b, c);
        const double w = wide_weight<W>(s, a, b, c) * s.coeff;
        v.dirty[node >> 4] = v.epoch;
        double *Fn = F + 3 * node;
        unsafeAtomicAdd(Fn, g0 * w); unsafeAtomicAdd(Fn + 1, g1 * w); unsafeAtomicAdd(Fn + 2, g2 * w);
      }
}

// v = sum over the admitted nodes, in visiting order, of u(node) * weight
template <int W>
__device__ __forceinline__ void wide_blend_global(const LatView &v, const PopView &pv, const WStencil<W> &s, const WAxes<W> &ax, double out[3]) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
  for (int a = 0; a < W; a++)
#pragma unroll
    for (int b = 0; b < W; b++)
#pragma unroll
      for (int c = 0; c < W; c++) {
        if (!(s.adm & (1ull << ((a * W + b) * W + c)))) continue;
        double u[3];
        node_velocity<false>(v, pv, ax.l[0][a], ax.l[1][b], ax.l[2][c], wide_node<W>(v, ax, a, b, c), u);
        const double w = wide_weight<W>(s, a, b, c) * s.coeff;
        a0 += (u[0] * w); a1 += (u[1] * w); a2 += (u[2] * w);
      }
  out[0] = a0; out[1] = a1; out[2] = a2;
}

template <int W>
__global__ __launch_bounds__(256) void ibm_wide_interpolate_kernel(LatView v, PopView pv, long n, const double *px, const double *py, const double *pz,
                                                                   double *vx, double *vy, double *vz, const int *vert_cell, const int *tag, const unsigned char *dead) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag[vert_cell[i]] == 1) return;
  WStencil<W> s; WAxes<W> ax;
  wide_stencil<W>(v, px[i], py[i], pz[i], s, ax);
  double u[3];
  wide_blend_global<W>(v, pv, s, ax, u);
  vx[i] = u[0]; vy[i] = u[1]; vz[i] = u[2];
}

// entries of the reproducible spread (ibm.hip: spread_emit_kernel): W^3 per vertex from entry ebase on, in visiting order
template <int W>
__global__ __launch_bounds__(256) void wide_emit_kernel(LatView v, int nv, long n, const int *order, long ebase, const double *px, const double *py,
                                                        const double *pz, double *fx, double *fy, double *fz, const double *rx, const double *ry,
                                                        const double *rz, int limit_on, double f_limit, const int *tag, const unsigned char *dead,
                                                        unsigned int *keys, int *vals, double *c0, double *c1, double *c2) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;   // (rank of the cell in id order) * nv + vertex
  if (g >= n) return;
  const int cell = order[g / nv];
  const long i = (long)cell * nv + (g % nv);
  const long e0 = ebase + g * (W * W * W);
  const bool live = tag[cell] != 1 && !dead[i];
  WStencil<W> s; WAxes<W> ax;
  s.adm = 0; s.coeff = 0.0;
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  if (live) {
    f0 = fx[i]; f1 = fy[i]; f2 = fz[i];
    if (limit_on) {  // FORCE_LIMIT cap, core/hemoCellParticleField.cpp:848-852 (mutates sv.force)
      const double mag = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
      if (mag > f_limit) { const double sc = f_limit / mag; f0 *= sc; f1 *= sc; f2 *= sc; fx[i] = f0; fy[i] = f1; fz[i] = f2; }
    }
    if (rx) { f0 = rx[i] + f0; f1 = ry[i] + f1; f2 = rz[i] + f2; }   // force_repulsion + force, :857-859
    wide_stencil<W>(v, px[i], py[i], pz[i], s, ax);
  }
#pragma unroll
  for (int a = 0; a < W; a++)
#pragma unroll
    for (int b = 0; b < W; b++)
#pragma unroll
      for (int c = 0; c < W; c++) {
        const int k = (a * W + b) * W + c;
        const bool adm = (s.adm >> k) & 1ull;   // never set for a vertex that is not live
        double w = 0.0; unsigned int key = 0xffffffffu;
        if (adm) { w = wide_weight<W>(s, a, b, c) * s.coeff; key = (unsigned int)wide_node<W>(v, ax, a, b, c); }
        keys[e0 + k] = key;
        vals[e0 + k] = (int)(e0 + k);
        c0[e0 + k] = adm ? f0 * w : 0.0; c1[e0 + k] = adm ? f1 * w : 0.0; c2[e0 + k] = adm ? f2 * w : 0.0;
      }
}

// ----------------------------------------------------------------------------
// one workgroup per cell, on an LDS tile: the scheme of ibm.hip (tile, mask tile, compacted node list, ds_add_f64, one global
// fp64 atomic per touched node and component) with the caps of the width.  The mask tile is always filled: with 27 or 64 nodes
// per vertex its bytes are a small part of the work, and the wall-brick shortcut of ibm.hip would have to prove a box of 20^3 clear.

// local (wrapped) origin and decode reciprocals; false when the tile cannot be used
__device__ __forceinline__ bool wide_tile_finish(const LatView &v, Tile &t, int cap) {
  if (t.vol > cap) return false;
  if ((v.wrap_x && t.e[0] > v.nx) || (v.per_y && t.e[1] > v.ny) || (v.per_z && t.e[2] > v.nz)) return false;
  t.ow[0] = v.wrap_x ? (int)pmod((long)t.o[0] - v.x0, v.nx) : t.o[0] - v.x0;
  t.ow[1] = v.per_y ? (int)pmod(t.o[1], v.ny) : t.o[1];
  t.ow[2] = v.per_z ? (int)pmod(t.o[2], v.nz) : t.o[2];
  t.r1 = 1.0f / (float)t.e[1]; t.r2 = 1.0f / (float)t.e[2];
  return true;
}

// positions -> weight rows in registers, tile, mask tile, admission.  Returns false (uniformly) when the cell does not fit the
// tile and the caller must take the per-vertex path.  dead: removed particles of an INCOMPLETE cell (null for a complete one)
template <int W>
__device__ __forceinline__ bool wide_prologue(const LatView &v, int nv, long base, const double *px, const double *py, const double *pz,
                                              const unsigned char *dead, int *s_red, unsigned char *mt, Tile &t, WStencil<W> vs[NVPT]) {
  const int tid = threadIdx.x, nth = blockDim.x;
  int b[NVPT][3]; bool live[NVPT];
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    const int i = tid + j * nth;
    live[j] = i < nv && !(dead && dead[base + i]);
    vs[j].adm = 0; vs[j].base = 0; vs[j].coeff = 0.0;
    if (live[j]) {
      wide_rows<W>(px[base + i], py[base + i], pz[base + i], b[j], vs[j]);
#pragma unroll
      for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], b[j][a]); hi[a] = max(hi[a], b[j][a] + W - 1); }
    }
  }
  block_bbox(lo, hi, s_red, t);
  if (!wide_tile_finish(v, t, tile_cap<W>()) || nv > NVPT * nth) return false;
#pragma unroll 4
  for (int i = tid; i < t.vol; i += nth) mt[i] = tile_mask(v, t, i);
  __syncthreads();
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    if (!live[j]) continue;
    WStencil<W> &s = vs[j];
    s.base = ((b[j][0] - t.o[0]) * t.e[1] + (b[j][1] - t.o[1])) * t.e[2] + (b[j][2] - t.o[2]);
    double total = 0.0;
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
      for (int c = 0; c < W; c++)
#pragma unroll
        for (int k = 0; k < W; k++) {
          const double weight = wide_weight<W>(s, a, c, k);
          if (weight != 0.0 && mt[s.base + a * sx + c * sy + k] == 0) { total += weight; s.adm |= 1ull << ((a * W + c) * W + k); }
        }
    s.coeff = 1.0 / total;
  }
  return true;
}

// Compacts the nodes the cell's stencils admit, as compact_nodes of ibm.hip does: slot[tile index] = rank of the node,
// list[rank] = tile index.  Returns the node count (uniform); above the cap the list is incomplete.
constexpr unsigned short SLOT_FREE = 0xFFFF, SLOT_MARK = 0xFFFE;
template <int W>
__device__ __forceinline__ int wide_compact(const Tile &t, const WStencil<W> vs[NVPT], unsigned short *slot, unsigned short *list, int *s_count) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
  for (int i = tid; i < t.vol; i += nth) slot[i] = SLOT_FREE;
  if (tid == 0) *s_count = 0;
  __syncthreads();   // also: every thread is done reading the mask tile, list may overwrite it
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    if (!vs[j].adm) continue;
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
      for (int c = 0; c < W; c++)
#pragma unroll
        for (int k = 0; k < W; k++)
          if (vs[j].adm & (1ull << ((a * W + c) * W + k))) slot[vs[j].base + a * sx + c * sy + k] = SLOT_MARK;
  }
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
      if (n < node_cap<W>()) { slot[i] = (unsigned short)n; list[n] = (unsigned short)i; }
    }
  }
  __syncthreads();
  return *s_count;
}

// per-vertex spread with direct global atomics: cells larger than the tile or touching more nodes than the cap
template <int W>
__device__ void wide_spread_direct(const LatView &v, int nv, long base, const double *px, const double *py, const double *pz, const double *fx,
                                   const double *fy, const double *fz, const double *rx, const double *ry, const double *rz, double *F,
                                   const unsigned char *dead) {
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    if (dead && dead[base + i]) continue;
    WStencil<W> s; WAxes<W> ax;
    wide_stencil<W>(v, px[base + i], py[base + i], pz[base + i], s, ax);
    const double f0 = (rx ? rx[base + i] : 0.0) + fx[base + i], f1 = (ry ? ry[base + i] : 0.0) + fy[base + i], f2 = (rz ? rz[base + i] : 0.0) + fz[base + i];
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
      for (int b = 0; b < W; b++)
#pragma unroll
        for (int c = 0; c < W; c++) {
          if (!(s.adm & (1ull << ((a * W + b) * W + c)))) continue;
          const long node = wide_node<W>(v, ax, a, b, c);
          const double w = wide_weight<W>(s, a, b, c) * s.coeff;
          v.dirty[node >> 4] = v.epoch;
          double *Fn = F + 3 * node;
          unsafeAtomicAdd(Fn, f0 * w); unsafeAtomicAdd(Fn + 1, f1 * w); unsafeAtomicAdd(Fn + 2, f2 * w);
        }
  }
}

template <int W>
__global__ __launch_bounds__(256) void ibm_wide_spread_cell_kernel(LatView v, int nv, const double *px, const double *py, const double *pz,
                                                                   double *fx, double *fy, double *fz, const double *rx, const double *ry, const double *rz,
                                                                   double *F, int limit_on, double f_limit, const int *tag, const unsigned char *vdead) {
  constexpr int TC = tile_cap<W>(), NC = node_cap<W>();
  // 16-bit slots, the node list reuses the mask tile, the three force components of a touched node side by side (the layout of F)
  __shared__ unsigned short slot[TC];
  __shared__ __attribute__((aligned(16))) unsigned char raw[TC > 2 * NC ? TC : 2 * NC];
  unsigned char *mt = raw; unsigned short *list = reinterpret_cast<unsigned short *>(raw);
  __shared__ double acc[3 * NC];
  __shared__ int s_red[6 * MAXW], s_count;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int cell = (int)blockIdx.x;
  const int state = tag[cell];
  if (state == 1) return;                                        // the cell is gone
  const unsigned char *dead = state == 2 ? vdead : nullptr;      // incomplete: skip its removed particles
  const long base = (long)cell * nv;
  const bool in_regs = nv <= NVPT * nth;
  double f[NVPT][3];
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < NVPT; j++) {
      const int i = tid + j * nth;
      f[j][0] = f[j][1] = f[j][2] = 0.0;
      if (i < nv) { f[j][0] = fx[base + i]; f[j][1] = fy[base + i]; f[j][2] = fz[base + i]; }
    }
  }
  Tile t; WStencil<W> vs[NVPT];
  const bool tiled = wide_prologue<W>(v, nv, base, px, py, pz, dead, s_red, mt, t, vs);
  // FORCE_LIMIT cap, core/hemoCellParticleField.cpp:848-852 (mutates sv.force)
  if (limit_on) {
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < NVPT; j++) {
        const int i = tid + j * nth;
        if (i < nv && !(dead && dead[base + i])) {   // a removed particle is not in the list: its force stays
          const double mag = sqrt((f[j][0] * f[j][0] + f[j][1] * f[j][1]) + f[j][2] * f[j][2]);
          if (mag > f_limit) { const double sc = f_limit / mag; f[j][0] *= sc; f[j][1] *= sc; f[j][2] *= sc; fx[base + i] = f[j][0]; fy[base + i] = f[j][1]; fz[base + i] = f[j][2]; }
        }
      }
    } else {
      for (int i = tid; i < nv; i += nth) {
        if (dead && dead[base + i]) continue;
        const double f0 = fx[base + i], f1 = fy[base + i], f2 = fz[base + i];
        const double mag = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
        if (mag > f_limit) { const double sc = f_limit / mag; fx[base + i] = f0 * sc; fy[base + i] = f1 * sc; fz[base + i] = f2 * sc; }
      }
    }
  }
  const int n = tiled ? wide_compact<W>(t, vs, slot, list, &s_count) : 0;
  if (!tiled || n > NC) { wide_spread_direct<W>(v, nv, base, px, py, pz, fx, fy, fz, rx, ry, rz, F, dead); return; }   // uniform
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
  for (int k = tid; k < 3 * n; k += nth) acc[k] = 0.0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    const int i = tid + j * nth;
    if (i >= nv || !vs[j].adm) continue;
    double fv[3];   // force_repulsion + force, :857-859
    fv[0] = (rx ? rx[base + i] : 0.0) + f[j][0]; fv[1] = (ry ? ry[base + i] : 0.0) + f[j][1]; fv[2] = (rz ? rz[base + i] : 0.0) + f[j][2];
#pragma unroll
    for (int a = 0; a < W; a++)
#pragma unroll
      for (int c = 0; c < W; c++)
#pragma unroll
        for (int k = 0; k < W; k++) {
          if (!(vs[j].adm & (1ull << ((a * W + c) * W + k)))) continue;
          const double w = wide_weight<W>(vs[j], a, c, k) * vs[j].coeff;
          double *q = &acc[3 * slot[vs[j].base + a * sx + c * sy + k]];
          atomicAdd(q, fv[0] * w); atomicAdd(q + 1, fv[1] * w); atomicAdd(q + 2, fv[2] * w);
        }
  }
  __syncthreads();
  for (int k = tid; k < 3 * n; k += nth) {
    const double val = acc[k];
    if (val != 0.0) {
      const int q = k / 3;
      int lx, ly, lz; const long node = tile_node(v, t, list[q], lx, ly, lz); v.dirty[node >> 4] = v.epoch;
      unsafeAtomicAdd(&F[3 * node + (k - 3 * q)], val);
    }
  }
}

template <int W>
__global__ __launch_bounds__(256) void ibm_wide_interpolate_cell_kernel(LatView v, PopView pv, int nv, const double *px, const double *py, const double *pz,
                                                                        double *vx, double *vy, double *vz, const int *slots, const int *tag, const unsigned char *vdead) {
  constexpr int TC = tile_cap<W>(), NC = node_cap<W>();
  __shared__ unsigned short slot[TC];
  __shared__ __attribute__((aligned(16))) unsigned char raw[TC > 2 * NC ? TC : 2 * NC];
  unsigned char *mt = raw; unsigned short *list = reinterpret_cast<unsigned short *>(raw);
  __shared__ double ux[NC], uy[NC], uz[NC];
  __shared__ int s_red[6 * MAXW], s_count;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int cell = slots ? slots[blockIdx.x] : (int)blockIdx.x;   // slots: only the listed cells of the type
  const int state = tag[cell];
  if (state == 1) return;
  const unsigned char *dead = state == 2 ? vdead : nullptr;
  const long base = (long)cell * nv;
  Tile t; WStencil<W> vs[NVPT];
  bool tiled = wide_prologue<W>(v, nv, base, px, py, pz, dead, s_red, mt, t, vs);
  if (tiled && wide_compact<W>(t, vs, slot, list, &s_count) > NC) tiled = false;   // uniform: s_count is shared
  if (tiled) {
    const int sy = t.e[2], sx = t.e[1] * t.e[2];
    const int n = s_count;
    for (int k = tid; k < n; k += nth) {       // node velocity once per node
      int lx, ly, lz;
      const long node = tile_node(v, t, list[k], lx, ly, lz);
      double u[3];
      node_velocity<false>(v, pv, lx, ly, lz, node, u);
      ux[k] = u[0]; uy[k] = u[1]; uz[k] = u[2];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NVPT; j++) {
      const int i = tid + j * nth;
      if (i >= nv || (dead && dead[base + i])) continue;   // a removed particle keeps its velocity, as in the per-vertex forms
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int a = 0; a < W; a++)
#pragma unroll
        for (int c = 0; c < W; c++)
#pragma unroll
          for (int k = 0; k < W; k++) {
            if (!(vs[j].adm & (1ull << ((a * W + c) * W + k)))) continue;
            const int q = slot[vs[j].base + a * sx + c * sy + k];
            const double w = wide_weight<W>(vs[j], a, c, k) * vs[j].coeff;
            a0 += (ux[q] * w); a1 += (uy[q] * w); a2 += (uz[q] * w);
          }
      vx[base + i] = a0; vy[base + i] = a1; vz[base + i] = a2;
    }
    return;
  }
  for (int i = tid; i < nv; i += nth) {   // per-vertex gathers
    if (dead && dead[base + i]) continue;
    WStencil<W> s; WAxes<W> ax;
    wide_stencil<W>(v, px[base + i], py[base + i], pz[base + i], s, ax);
    double u[3];
    wide_blend_global<W>(v, pv, s, ax, u);
    vx[base + i] = u[0]; vy[base + i] = u[1]; vz[base + i] = u[2];
  }
}

}  // namespace

namespace hcc {

int wide_spread(hc_cells *C, int t, int force_limit, int per_vertex) {
  const LatView v = make_view(C->L);
  const int nv = C->types[t]->host.nv, W = C->ibm_kernel[t];
  const long n = C->ncells[t] * nv;
  const TypeArrays a = vert_arrays(C, t);   // r is set exactly when rep_on(), see vert_arrays
  double *F = C->L->force[C->L->fcur];
  if (per_vertex) {
    const dim3 grid((unsigned)((n + 255) / 256));
    auto go = [&](auto K) { hipLaunchKernelGGL(K, grid, dim3(256), 0, hc::stream(), v, n, a.p[0], a.p[1], a.p[2], a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2],
                                               F, force_limit, C->P.f_limit, a.vert_cell, a.tag_all, a.dead); };
    if (W == HC_IBM_PHI3) go(ibm_wide_spread_kernel<3>); else go(ibm_wide_spread_kernel<4>);
  } else {
    auto go = [&](auto K) { hipLaunchKernelGGL(K, dim3((unsigned)C->ncells[t]), dim3(nv > 128 ? 256 : 128), 0, hc::stream(), v, nv, a.p[0], a.p[1], a.p[2],
                                               a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2], F, force_limit, C->P.f_limit, a.tag, a.dead); };
    if (W == HC_IBM_PHI3) go(ibm_wide_spread_cell_kernel<3>); else go(ibm_wide_spread_cell_kernel<4>);
  }
  HC_HIP(hipGetLastError());
  return HC_OK;
}

int wide_interpolate(hc_cells *C, int t, const int *slots, int n_slots, int per_vertex) {
  const hc_lattice *L = C->L;
  HC_REQUIRE(L->ob_n == 0 && L->n_slabs == 1, "hcp_interpolate: a three- or four-point IBM kernel on a lattice with open boundaries or slabs");   // refused at set-up, both ways
  const LatView v = make_view(L);
  const PopView pv = make_pops(L);
  const int nv = C->types[t]->host.nv, W = C->ibm_kernel[t];
  const long n = C->ncells[t] * nv;
  const TypeArrays a = vert_arrays(C, t);
  if (per_vertex && !slots) {
    const dim3 grid((unsigned)((n + 255) / 256));
    auto go = [&](auto K) { hipLaunchKernelGGL(K, grid, dim3(256), 0, hc::stream(), v, pv, n, a.p[0], a.p[1], a.p[2], a.v[0], a.v[1], a.v[2],
                                               a.vert_cell, a.tag_all, a.dead); };
    if (W == HC_IBM_PHI3) go(ibm_wide_interpolate_kernel<3>); else go(ibm_wide_interpolate_kernel<4>);
  } else {
    const unsigned cells = slots ? (unsigned)n_slots : (unsigned)C->ncells[t];
    auto go = [&](auto K) { hipLaunchKernelGGL(K, dim3(cells), dim3(nv > 128 ? 256 : 128), 0, hc::stream(), v, pv, nv, a.p[0], a.p[1], a.p[2], a.v[0], a.v[1], a.v[2],
                                               slots, a.tag, a.dead); };
    if (W == HC_IBM_PHI3) go(ibm_wide_interpolate_cell_kernel<3>); else go(ibm_wide_interpolate_cell_kernel<4>);
  }
  HC_HIP(hipGetLastError());
  return HC_OK;
}

int wide_emit(hc_cells *C, int t, const int *d_order, long ebase, int force_limit) {
  const LatView v = make_view(C->L);
  const int nv = C->types[t]->host.nv, W = C->ibm_kernel[t];
  const long n = C->ncells[t] * nv;
  const TypeArrays a = vert_arrays(C, t);
  auto go = [&](auto K) { hipLaunchKernelGGL(K, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, nv, n, d_order, ebase, a.p[0], a.p[1], a.p[2],
                                             a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2], force_limit, C->P.f_limit, a.tag, a.dead, C->det_keys[0], C->det_vals[0],
                                             C->det_val[0], C->det_val[1], C->det_val[2]); };
  if (W == HC_IBM_PHI3) go(wide_emit_kernel<3>); else go(wide_emit_kernel<4>);
  HC_HIP(hipGetLastError());
  return HC_OK;
}

}  // namespace hcc

extern "C" {

int hcp_type_set_ibm_kernel(hc_cells *C, int type, int kernel) {
  HC_REQUIRE(C && type >= 0 && type < C->ntypes, "hcp_type_set_ibm_kernel: unknown cell type");
  HC_REQUIRE(kernel == HC_IBM_PHI2 || kernel == HC_IBM_PHI3 || kernel == HC_IBM_PHI4, "hcp_type_set_ibm_kernel: kernel must be HC_IBM_PHI2, HC_IBM_PHI3 or HC_IBM_PHI4");
  const int old = C->ibm_kernel[type];
  if (kernel == old) return HC_OK;
  const hc_lattice *L = C->L;
  if (kernel != HC_IBM_PHI2) {
    HC_REQUIRE(L->n_slabs == 1, "hcp_type_set_ibm_kernel: a three- or four-point kernel needs the whole domain on one GPU (n_slabs = 1): four points need two halo planes");
    HC_REQUIRE(L->ob_n == 0, "hcp_type_set_ibm_kernel: the lattice has open-boundary nodes; those and a three- or four-point kernel do not combine");
    HC_REQUIRE(!hc::in_preinlet_pair(L), "hcp_type_set_ibm_kernel: the lattice is part of a pre-inlet pair; a pre-inlet and a three- or four-point kernel do not combine");
    HC_REQUIRE(!C->visc_class[type], "hcp_type_set_ibm_kernel: the type has interior viscosity, whose membrane pass walks the eight-node stencil");
  }
  if (old == HC_IBM_PHI2) hc::ibm_wide_add(C, L);
  else if (kernel == HC_IBM_PHI2) hc::ibm_wide_remove_one(C);
  C->ibm_kernel[type] = kernel;
  return HC_OK;
}

int hcp_type_get_ibm_kernel(hc_cells *C, int type, int *kernel) {
  HC_REQUIRE(C && kernel && type >= 0 && type < C->ntypes, "hcp_type_get_ibm_kernel: bad arguments");
  *kernel = C->ibm_kernel[type];
  return HC_OK;
}

}  // extern "C"
