// Immersed-boundary coupling on the GPU: phi2 force spreading and velocity interpolation.
//
// Replaces (file:line in the HemoCell tree):
//   core/immersedBoundaryMethod.h:62-138          interpolationCoefficientsPhi2 (cells.h: phi2_stencil)
//   core/hemoCellParticleField.cpp:841-863        spreadParticleForce
//   core/hemoCellParticleField.cpp:819-839        interpolateFluidVelocity
#include "ibm_common.h"
#include <hipcub/hipcub.hpp>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace {

// ----------------------------------------------------------------------------
// spread
__global__ __launch_bounds__(256) void ibm_spread_kernel(LatView v, long n, const double *px, const double *py, const double *pz,
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
  Stencil s;
  phi2_stencil(v, px[i], py[i], pz[i], s);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (s.node[k] < 0) continue;
    v.dirty[s.node[k] >> 4] = v.epoch;
    // external.data[d] += (force_repulsion[d] + force[d]) * weight  (:857-859)
    double *Fn = F + 3 * s.node[k];
    unsafeAtomicAdd(Fn, ((rx ? rx[i] : 0.0) + f0) * s.w[k]);
    unsafeAtomicAdd(Fn + 1, ((ry ? ry[i] : 0.0) + f1) * s.w[k]);
    unsafeAtomicAdd(Fn + 2, ((rz ? rz[i] : 0.0) + f2) * s.w[k]);
  }
}

// ----------------------------------------------------------------------------
// reproducible spread (hc_set_reproducible_spread).  The reference adds particle by particle in storage order
// (core/hemoCellParticleField.cpp:841-863), so a node's force is a sum in a fixed order and a run repeats bit for bit; the
// atomic kernels above add in whatever order the hardware takes them.  Here every (particle, admitted stencil node) becomes an
// entry keyed by its node, written in the canonical order (cell type, cell id, vertex id, stencil node); a stable radix
// sort by node groups the entries of a node without disturbing that order, and ONE thread per node sums them in sequence and
// adds the sum to the node.  The order does not depend on the storage slots of the cells, so every slab that holds a node
// forms the bits the single domain forms.
__global__ __launch_bounds__(256) void spread_emit_kernel(LatView v, int nv, long n, const int *order, long ebase, const double *px, const double *py,
                                                          const double *pz, double *fx, double *fy, double *fz, const double *rx, const double *ry,
                                                          const double *rz, int limit_on, double f_limit, const int *tag, const unsigned char *dead,
                                                          unsigned int *keys, int *vals, double *c0, double *c1, double *c2) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;   // (rank of the cell in id order) * nv + vertex
  if (g >= n) return;
  const int cell = order[g / nv];
  const long i = (long)cell * nv + (g % nv);
  const long e0 = (ebase + g) * 8;
  const bool live = tag[cell] != 1 && !dead[i];
  Stencil s;
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  if (live) {
    f0 = fx[i]; f1 = fy[i]; f2 = fz[i];
    if (limit_on) {  // FORCE_LIMIT cap, core/hemoCellParticleField.cpp:848-852 (mutates sv.force)
      const double mag = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
      if (mag > f_limit) { const double sc = f_limit / mag; f0 *= sc; f1 *= sc; f2 *= sc; fx[i] = f0; fy[i] = f1; fz[i] = f2; }
    }
    if (rx) { f0 = rx[i] + f0; f1 = ry[i] + f1; f2 = rz[i] + f2; }   // force_repulsion + force, :857-859
    phi2_stencil(v, px[i], py[i], pz[i], s);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const bool adm = live && s.node[k] >= 0;
    keys[e0 + k] = adm ? (unsigned int)s.node[k] : 0xffffffffu;
    vals[e0 + k] = (int)(e0 + k);
    c0[e0 + k] = adm ? f0 * s.w[k] : 0.0; c1[e0 + k] = adm ? f1 * s.w[k] : 0.0; c2[e0 + k] = adm ? f2 * s.w[k] : 0.0;
  }
}

__global__ __launch_bounds__(256) void spread_gather_kernel(LatView v, long n, const unsigned int *keys, const int *vals, const double *c0, const double *c1,
                                                            const double *c2, double *F) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const unsigned int key = keys[s];
  if (key == 0xffffffffu || (s > 0 && keys[s - 1] == key)) return;   // not the first entry of its node
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (long q = s; q < n && keys[q] == key; q++) { const int e = vals[q]; a0 += c0[e]; a1 += c1[e]; a2 += c2[e]; }
  v.dirty[key >> 4] = v.epoch;
  double *Fn = F + 3 * (long)key;
  Fn[0] += a0; Fn[1] += a1; Fn[2] += a2;   // this thread alone touches the node
}


// node velocities of one face plane of a slab (lx = 0 or nx - 1), for the neighbour whose first halo plane it is.  OPEN: a fluid
// open-boundary node of the plane sends the moments of its completed populations (a velocity node u_bc + F / 2), the rule the
// neighbour's interpolation follows for its own nodes; with plain moments the unknown populations would count as zeros
template <bool OPEN = false>
__global__ __launch_bounds__(256) void face_velocity_kernel(LatView v, Pops<OPEN> pv, int lx0, double *out0, int lx1, double *out1) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= v.ny_nz) return;
  const int lx = blockIdx.y ? lx1 : lx0;           // blockIdx.y: which of the (up to two) planes of the launch
  double *out = blockIdx.y ? out1 : out0;
  const int ly = k / v.nz, lz = k - ly * v.nz;
  const long node = (long)(lx + HALO) * v.plane + (long)ly * v.nz + lz;
  double u[3] = {0.0, 0.0, 0.0};
  if (v.mask[node] == 0) node_velocity<OPEN>(v, pv, lx, ly, lz, node, u);   // stencils admit fluid nodes only
  out[k] = u[0]; out[v.ny_nz + k] = u[1]; out[2L * v.ny_nz + k] = u[2];
}

template <bool OPEN = false>
__global__ __launch_bounds__(256) void ibm_interpolate_kernel(LatView v, Pops<OPEN> pv, long n, const double *px, const double *py,
                                                              const double *pz, double *vx, double *vy, double *vz, const int *vert_cell, const int *tag,
                                                              const unsigned char *dead) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag[vert_cell[i]] == 1) return;
  Stencil s;
  phi2_stencil(v, px[i], py[i], pz[i], s);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (s.node[k] < 0) continue;
    double u[3];
    node_velocity<OPEN>(v, pv, s.lx[k], s.ly[k], s.lz[k], s.node[k], u);
    a0 += (u[0] * s.w[k]); a1 += (u[1] * s.w[k]); a2 += (u[2] * s.w[k]);
  }
  vx[i] = a0; vy[i] = a1; vz[i] = a2;
}


// ----------------------------------------------------------------------------
// LDS-tiled IBM kernels: one workgroup per cell.
//
// All 8-node stencils of a cell fall into the cell's bounding box (+1); the nodes the cell touches are compacted
// into a list (compact_nodes).  Spread: the workgroup accumulates the three force components per listed node in
// LDS (ds_add_f64), then flushes them to HBM with one fp64 atomic per (node, component) -- several times fewer,
// better shaped global atomics than one per (vertex, node, component).  Interpolate: the node velocity
// (19-population gather + moments) is evaluated once per listed node into LDS, and every vertex then blends its
// 8 values from LDS.
constexpr int TILE_CAP = 5832;       // nodes per tile: 18 x 18 x 18, any orientation of a 642-vertex RBC; three workgroups per CU fit the 160 KB LDS
constexpr int NODE_CAP = 1536;       // distinct nodes of one cell for the interpolation (an RBC touches ~1300)


__device__ __forceinline__ int stencil_base(const LatView &v, double px, double py, double pz, int b[3]) {
  const double p[3] = {px, py, pz};
#pragma unroll
  for (int a = 0; a < 3; a++) { const long c = nearest_node(p[a]); b[a] = (int)c + ((p[a] < (double)c) ? -1 : 0); }
  return 0;
}


// Workgroups are handed to the 8 XCDs round robin, and every XCD has its own L2.  Cells are stored in placement order,
// neighbours in space mostly next to each other; giving each XCD a contiguous range of cells lets neighbouring cells,
// which share the lattice lines around their common boundary, meet in one L2 (interpolation -3 %, spread -1 % on the
// 256^3 pipe, three runs each way).
__device__ __forceinline__ int xcd_contiguous(int b, int n) {
  const int per = n >> 3;            // cells per XCD in the swizzled part
  const int main_n = per << 3;
  if (b >= main_n) return b;          // the remainder keeps its place
  return (b & 7) * per + (b >> 3);
}

// compact per-vertex stencil kept in registers across the passes of the cell kernels
struct VStencil { double w[8]; int base; unsigned adm; };   // base = tile index of the lowest corner; adm = admitted-node bits

constexpr int NVPT = 3;        // vertices per thread held in registers (642 vertices / 256 threads)
// Four waves per workgroup (MAXW, ibm_common.h).  Eight waves per cell (512 threads, two vertices each) were tried for both kernels: the spread gains 3.5 % at 10 % hematocrit
// and nothing at 25 % (and loses once its loads are reordered), the interpolation loses 9-15 % (184 VGPRs: one cell per CU);
// capping the interpolation at 168 / 128 VGPRs for three cells per CU spills and loses 15 %.  Both kernels wait 80 % of their
// wave cycles (rocprofv3 SQ_WAIT_ANY + SQ_WAIT_INST_ANY) and respond to neither more waves nor shorter workgroups.

// -DHC_IBM_PHASE_TIMES (scratch builds only): thread 0 of every workgroup adds the shader cycles between consecutive stamps to
// g_phase[k]; hc_debug_phase_times() reads and clears them
#ifdef HC_IBM_PHASE_TIMES
__device__ unsigned long long g_phase[32];
#define PH_PARAM , long long &ph_last
#define PH_ARG , ph_last
#define PH_INIT long long ph_last = clock64();
#define STAMP(k) do { if (threadIdx.x == 0) { const long long ph_now = clock64(); atomicAdd(&g_phase[k], (unsigned long long)(ph_now - ph_last)); ph_last = ph_now; } } while (0)
#else
#define PH_PARAM
#define PH_ARG
#define PH_INIT
#define STAMP(k) do {} while (0)
#endif


// local (wrapped) origin and decode reciprocals; false when the tile cannot be used
__device__ __forceinline__ bool tile_finish(const LatView &v, Tile &t) {
  if (t.vol > TILE_CAP) return false;
  if ((v.wrap_x && t.e[0] > v.nx) || (v.per_y && t.e[1] > v.ny) || (v.per_z && t.e[2] > v.nz)) return false;
  t.ow[0] = v.wrap_x ? (int)pmod((long)t.o[0] - v.x0, v.nx) : t.o[0] - v.x0;
  t.ow[1] = v.per_y ? (int)pmod(t.o[1], v.ny) : t.o[1];
  t.ow[2] = v.per_z ? (int)pmod(t.o[2], v.nz) : t.o[2];
  t.r1 = 1.0f / (float)t.e[1]; t.r2 = 1.0f / (float)t.e[2];
  return true;
}


// interpolationCoefficientsPhi2 against the LDS copy of the mask; same arithmetic and visiting order as phi2_stencil
__device__ __forceinline__ void tile_stencil(const Tile &t, const unsigned char *mt, double px, double py, double pz, const int b[3], VStencil &o) {
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
        const double weight = phi2(px - (double)(b[0] + i)) * phi2(py - (double)(b[1] + j)) * phi2(pz - (double)(b[2] + k));
        const bool adm = (weight != 0.0) && (!mt || mt[o.base + i * sx + j * sy + k] == 0);   // mt == nullptr: no wall anywhere near this cell
        if (adm) { total += weight; o.adm |= 1u << idx; }
        o.w[idx] = adm ? weight : 0.0;
      }
  const double coeff = 1.0 / total;
#pragma unroll
  for (int idx = 0; idx < 8; idx++) o.w[idx] *= coeff;
}

// Is every node of the tile an ordinary fluid node inside the domain?  Then interpolationCoefficientsPhi2 admits every node
// with a non-zero weight and the mask need not be looked at (most cells of a vessel are nowhere near its wall).  Answered
// from one byte per 8 x 8 x 8 brick of the padded lattice (hc_lattice::wallbrick: set when the brick holds a non-fluid node or
// touches a face the stencils cannot cross); a tile covers at most 4 x 4 x 4 bricks, one per lane of wave 0.
__device__ __forceinline__ bool tile_is_clear(const LatView &v, const Tile &t, int *s_near) {
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
    if (l == 0) *s_near = any != 0ull;
  }
  __syncthreads();
  return *s_near == 0;
}

// shared prologue of the two cell kernels: positions -> registers, tile, mask tile (only near walls), stencils.
// returns false (uniformly) when the cell does not fit the tile and the caller must take the fallback path
// dead: removed particles of an INCOMPLETE cell (null for a complete one); they take no part in anything
__device__ __forceinline__ bool cell_prologue(const LatView &v, int nv, long base, const double *px, const double *py, const double *pz,
                                              const unsigned char *dead, int *s_red, int *s_near, unsigned char *mt, Tile &t, VStencil vs[NVPT] PH_PARAM) {
  const int tid = threadIdx.x, nth = blockDim.x;
  double p[NVPT][3]; int b[NVPT][3]; bool live[NVPT];
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    const int i = tid + j * nth;
    live[j] = i < nv && !(dead && dead[base + i]);
    if (live[j]) {
      p[j][0] = px[base + i]; p[j][1] = py[base + i]; p[j][2] = pz[base + i];
      stencil_base(v, p[j][0], p[j][1], p[j][2], b[j]);
#pragma unroll
      for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], b[j][a]); hi[a] = max(hi[a], b[j][a] + 1); }
    }
  }
  block_bbox(lo, hi, s_red, t);
  STAMP(1);
  if (!tile_finish(v, t) || nv > NVPT * nth) return false;
  const bool clear = tile_is_clear(v, t, s_near);   // uniform
  STAMP(2);
  if (!clear) {
#pragma unroll 4
    for (int i = tid; i < t.vol; i += nth) mt[i] = tile_mask(v, t, i);
    __syncthreads();
  }
  STAMP(3);
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    vs[j].adm = 0; vs[j].base = 0;
    if (live[j]) tile_stencil(t, clear ? nullptr : mt, p[j][0], p[j][1], p[j][2], b[j], vs[j]);
  }
  STAMP(4);
  return true;
}

// Compacts the nodes the cell's stencils admit: slot[tile index] = rank of the node, list[rank] = tile index, in tile order within
// each wave's 256 tile entries (runs along z stay runs).  One LDS atomic per wave, ranks within the wave from its ballot.  Returns
// the node count (uniform); a count above NODE_CAP means the list is incomplete and the caller takes its fallback path.
constexpr unsigned short SLOT_FREE = 0xFFFF, SLOT_MARK = 0xFFFE;
__device__ __forceinline__ int compact_nodes(const Tile &t, const VStencil vs[NVPT], unsigned short *slot, unsigned short *list, int *s_count) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
  for (int i = tid; i < t.vol; i += nth) slot[i] = SLOT_FREE;
  if (tid == 0) *s_count = 0;
  __syncthreads();   // also: every thread is done reading the mask tile, list may overwrite it
#pragma unroll
  for (int j = 0; j < NVPT; j++)   // mark the admitted nodes
#pragma unroll
    for (int k = 0; k < 8; k++) if (vs[j].adm & (1u << k)) slot[vs[j].base + (k >> 2) * sx + ((k >> 1) & 1) * sy + (k & 1)] = SLOT_MARK;
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
      if (n < NODE_CAP) { slot[i] = (unsigned short)n; list[n] = (unsigned short)i; }
    }
  }
  __syncthreads();
  return *s_count;
}

// per-vertex spread with direct global atomics: cells larger than the tile or touching more than NODE_CAP nodes
__device__ void spread_direct(const LatView &v, int nv, long base, const double *px, const double *py, const double *pz, const double *fx,
                              const double *fy, const double *fz, const double *rx, const double *ry, const double *rz, double *F,
                              const unsigned char *dead) {
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    if (dead && dead[base + i]) continue;
    Stencil s;
    phi2_stencil(v, px[base + i], py[base + i], pz[base + i], s);
    const double f0 = (rx ? rx[base + i] : 0.0) + fx[base + i], f1 = (ry ? ry[base + i] : 0.0) + fy[base + i], f2 = (rz ? rz[base + i] : 0.0) + fz[base + i];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (s.node[k] < 0) continue;
      v.dirty[s.node[k] >> 4] = v.epoch;
      double *Fn = F + 3 * s.node[k];
      unsafeAtomicAdd(Fn, f0 * s.w[k]);
      unsafeAtomicAdd(Fn + 1, f1 * s.w[k]);
      unsafeAtomicAdd(Fn + 2, f2 * s.w[k]);
    }
  }
}

__global__ __launch_bounds__(256) void ibm_spread_cell_kernel(LatView v, int nv, const double *px, const double *py, const double *pz,
                                                              double *fx, double *fy, double *fz, const double *rx, const double *ry, const double *rz,
                                                              double *F, int limit_on, double f_limit, int xcd_ranges, const int *tag, const unsigned char *vdead) {
  // 54 KB in all, so that three workgroups share a CU: 16-bit slots, the node list reuses the mask tile, and the three force
  // components of a touched node side by side (acc[3 * rank + component], the layout of F)
  __shared__ unsigned short slot[TILE_CAP];
  __shared__ __attribute__((aligned(16))) unsigned char raw[TILE_CAP > 2 * NODE_CAP ? TILE_CAP : 2 * NODE_CAP];
  unsigned char *mt = raw; unsigned short *list = reinterpret_cast<unsigned short *>(raw);
  __shared__ double acc[3 * NODE_CAP];
  __shared__ int s_red[6 * MAXW], s_count, s_near;
  const int tid = threadIdx.x, nth = blockDim.x;
  PH_INIT
  const int cell = xcd_ranges ? xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int state = tag[cell];
  if (state == 1) return;                                        // the cell is gone
  STAMP(0);
  const unsigned char *dead = state == 2 ? vdead : nullptr;      // incomplete: skip its removed particles
  const long base = (long)cell * nv;
  const bool in_regs = nv <= NVPT * nth;
  // forces of this thread's vertices: the loads are issued here, together with the position loads of the prologue (nothing
  // is stored in between, so both travel in one round trip); the FORCE_LIMIT cap follows once the tile is known
  double f[NVPT][3];
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < NVPT; j++) {
      const int i = tid + j * nth;
      f[j][0] = f[j][1] = f[j][2] = 0.0;
      if (i < nv) { f[j][0] = fx[base + i]; f[j][1] = fy[base + i]; f[j][2] = fz[base + i]; }
    }
  }
  Tile t; VStencil vs[NVPT];
  bool tiled = cell_prologue(v, nv, base, px, py, pz, dead, s_red, &s_near, mt, t, vs PH_ARG);
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
  // The touched nodes are compacted and all three components accumulated per node in LDS (ds_add_f64), then flushed with one
  // fp64 atomic per (node, component), consecutive lanes on consecutive addresses: a z-run of a membrane across a row leaves as
  // one 48-96 byte segment of F instead of three 16-32 byte segments in three component planes.
  const int n = tiled ? compact_nodes(t, vs, slot, list, &s_count) : 0;
  STAMP(5);
  if (!tiled || n > NODE_CAP) { spread_direct(v, nv, base, px, py, pz, fx, fy, fz, rx, ry, rz, F, dead); return; }   // uniform
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
    for (int k = 0; k < 8; k++) {
      if (!(vs[j].adm & (1u << k))) continue;
      double *a = &acc[3 * slot[vs[j].base + (k >> 2) * sx + ((k >> 1) & 1) * sy + (k & 1)]];
      atomicAdd(a, fv[0] * vs[j].w[k]); atomicAdd(a + 1, fv[1] * vs[j].w[k]); atomicAdd(a + 2, fv[2] * vs[j].w[k]);
    }
  }
  __syncthreads();
  STAMP(6);
  for (int k = tid; k < 3 * n; k += nth) {
    const double val = acc[k];
    if (val != 0.0) {
      const int q = k / 3;
      int lx, ly, lz; const long node = tile_node(v, t, list[q], lx, ly, lz); v.dirty[node >> 4] = v.epoch;
      unsafeAtomicAdd(&F[3 * node + (k - 3 * q)], val);
    }
  }
  STAMP(7);
}

template <bool OPEN = false>
__global__ __launch_bounds__(256) void ibm_interpolate_cell_kernel(LatView v, Pops<OPEN> pv, int nv, const double *px, const double *py,
                                                                   const double *pz, double *vx, double *vy, double *vz, const int *slots, int xcd_ranges,
                                                                   const int *tag, const unsigned char *vdead) {
  // 54 KB in all, so that three workgroups share a CU: 16-bit slots, and the node list reuses the mask tile
  // (the mask is only read while the stencils are formed)
  __shared__ unsigned short slot[TILE_CAP];
  __shared__ __attribute__((aligned(16))) unsigned char raw[TILE_CAP > 2 * NODE_CAP ? TILE_CAP : 2 * NODE_CAP];
  unsigned char *mt = raw; unsigned short *list = reinterpret_cast<unsigned short *>(raw);
  __shared__ double ux[NODE_CAP], uy[NODE_CAP], uz[NODE_CAP];
  __shared__ int s_red[6 * MAXW], s_count, s_near;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int cell = slots ? slots[blockIdx.x] : (xcd_ranges ? xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x);   // slots: only the listed cells of the type
  const int state = tag[cell];
  if (state == 1) return;
  const unsigned char *dead = state == 2 ? vdead : nullptr;
  const long base = (long)cell * nv;
  Tile t; VStencil vs[NVPT];
  PH_INIT
  bool tiled = cell_prologue(v, nv, base, px, py, pz, dead, s_red, &s_near, mt, t, vs PH_ARG);
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
  if (tiled) {
    if (compact_nodes(t, vs, slot, list, &s_count) > NODE_CAP) tiled = false;   // uniform: s_count is shared
    STAMP(12);
  }
  if (tiled) {
    const int n = s_count;
    for (int k = tid; k < n; k += nth) {       // node velocity once per node
      int lx, ly, lz;
      const long node = tile_node(v, t, list[k], lx, ly, lz);
      double u[3];
      node_velocity<OPEN>(v, pv, lx, ly, lz, node, u);
      ux[k] = u[0]; uy[k] = u[1]; uz[k] = u[2];
    }
    __syncthreads();
    STAMP(13);
#pragma unroll
    for (int j = 0; j < NVPT; j++) {
      const int i = tid + j * nth;
      if (i >= nv || (dead && dead[base + i])) continue;   // a removed particle keeps its velocity, as in the per-vertex forms
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        if (!(vs[j].adm & (1u << k))) continue;
        const int q = slot[vs[j].base + (k >> 2) * sx + ((k >> 1) & 1) * sy + (k & 1)];
        a0 += (ux[q] * vs[j].w[k]); a1 += (uy[q] * vs[j].w[k]); a2 += (uz[q] * vs[j].w[k]);
      }
      vx[base + i] = a0; vy[base + i] = a1; vz[base + i] = a2;
    }
    STAMP(14);
    return;
  }
  for (int i = tid; i < nv; i += nth) {   // fallback: per-vertex gathers
    if (dead && dead[base + i]) continue;
    Stencil s;
    phi2_stencil(v, px[base + i], py[base + i], pz[base + i], s);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (s.node[k] < 0) continue;
      double u[3];
      node_velocity<OPEN>(v, pv, s.lx[k], s.ly[k], s.lz[k], s.node[k], u);
      a0 += (u[0] * s.w[k]); a1 += (u[1] * s.w[k]); a2 += (u[2] * s.w[k]);
    }
    vx[base + i] = a0; vy[base + i] = a1; vz[base + i] = a2;
  }
}


}  // namespace

static int g_ibm_per_vertex = 0;  // 1: one thread per vertex with direct global atomics (kept for A/B and as reference)
extern "C" int hc_debug_ibm_per_vertex(int on) { g_ibm_per_vertex = on; return HC_OK; }
static int g_reproducible = -1;   // -1: not chosen yet (HEMOCELL_REPRODUCIBLE_SPREAD decides at first use)
static bool reproducible() {
  if (g_reproducible < 0) { const char *e = std::getenv("HEMOCELL_REPRODUCIBLE_SPREAD"); g_reproducible = (e && *e && *e != '0') ? 1 : 0; }
  return g_reproducible == 1;
}
extern "C" int hc_set_reproducible_spread(int on) { g_reproducible = on ? 1 : 0; return HC_OK; }

// the gather form of the spread: entries -> stable sort by node -> one sequential sum per node
static int spread_reproducible(hc_cells *C, int force_limit) {
  const LatView v = make_view(C->L);
  // entries: 8 per vertex of a type on two points, 27 or 64 on the wide kernels (ibm_wide.hip).  A type's entries start on a
  // multiple of 8, the unit spread_emit_kernel counts its base in; entries in between keep an invalid key
  long n_e = 0, first_e[8];
  for (int t = 0; t < C->ntypes; t++) {
    const long w = ibm_width(C, t);
    first_e[t] = n_e;
    n_e += (C->ncells[t] * C->types[t]->host.nv * w * w * w + 7) / 8 * 8;
  }
  HC_REQUIRE(v.npad * 3 < 0xffffffffL && n_e < 0x7fffffffL, "reproducible spread: lattice or vertex count beyond its 32-bit keys");
  int rc;
  if (n_e > C->det_cap) {
    HC_HIP(hipDeviceSynchronize());
    const long cap = n_e + n_e / 4 + 4096;
    C->det_cap = 0;
    for (int k = 0; k < 2; k++) if ((rc = C->det_keys[k].reserve((size_t)cap)) != HC_OK || (rc = C->det_vals[k].reserve((size_t)cap)) != HC_OK) return rc;
    for (int k = 0; k < 3; k++) if ((rc = C->det_val[k].reserve((size_t)cap)) != HC_OK) return rc;
    size_t tmp_bytes = 0;
    HC_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, C->det_keys[0].p, C->det_keys[1].p, C->det_vals[0].p, C->det_vals[1].p, (int)cap, 0, 32, hc::stream()));
    if ((rc = C->det_tmp.reserve(tmp_bytes)) != HC_OK) return rc;
    C->det_cap = cap;
  }
  // cell slots in ascending cell id, type by type: the canonical order of the entries
  std::vector<int> order((size_t)0);
  std::vector<long> obase((size_t)C->ntypes, 0);
  for (int t = 0; t < C->ntypes; t++) {
    const size_t nc = (size_t)C->ncells[t], o = order.size();
    obase[(size_t)t] = (long)o;
    order.resize(o + nc);
    std::iota(order.begin() + (long)o, order.end(), 0);
    const std::vector<long> &ids = C->host[t].ids;
    std::stable_sort(order.begin() + (long)o, order.end(), [&](int a, int b) { return ids[(size_t)a] < ids[(size_t)b]; });
  }
  int *d_order = nullptr;
  rc = stage_ints(C, 2, &d_order, order.data(), (int)order.size()); if (rc != HC_OK) return rc;
  if (C->ibm_wide_on()) HC_HIP(hipMemsetAsync(C->det_keys[0].p, 0xff, (size_t)n_e * sizeof(unsigned int), hc::stream()));   // the entries between two types
  for (int t = 0; t < C->ntypes; t++) {
    const int nv = C->types[t]->host.nv;
    const long n = C->ncells[t] * nv;
    if (n == 0) continue;
    if (ibm_width(C, t) != HC_IBM_PHI2) { if ((rc = wide_emit(C, t, d_order + obase[(size_t)t], first_e[t], force_limit)) != HC_OK) return rc; continue; }
    const long ebase = first_e[t] / 8;
    const TypeArrays a = vert_arrays(C, t);   // r is set exactly when rep_on(), see vert_arrays: hcp_spread has synchronised to the device
    hipLaunchKernelGGL(spread_emit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, nv, n, (const int *)(d_order + obase[(size_t)t]), ebase,
                       a.p[0], a.p[1], a.p[2], a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2], force_limit, C->P.f_limit, a.tag, a.dead, C->det_keys[0], C->det_vals[0],
                       C->det_val[0], C->det_val[1], C->det_val[2]);
    HC_HIP(hipGetLastError());
  }
  // only the bits a node index needs: 2^bits > npad, so the low bits of an invalid key (all ones) still sort behind every node
  int bits = 1;
  while (bits < 32 && (1L << bits) <= v.npad) bits++;
  size_t tmp = C->det_tmp.cap;
  HC_HIP(hipcub::DeviceRadixSort::SortPairs(C->det_tmp.p, tmp, C->det_keys[0].p, C->det_keys[1].p, C->det_vals[0].p, C->det_vals[1].p, (int)n_e, 0, bits, hc::stream()));
  hipLaunchKernelGGL(spread_gather_kernel, dim3((unsigned)((n_e + 255) / 256)), dim3(256), 0, hc::stream(), v, n_e, (const unsigned int *)C->det_keys[1],
                     (const int *)C->det_vals[1], (const double *)C->det_val[0], (const double *)C->det_val[1], (const double *)C->det_val[2], C->L->force[C->L->fcur]);
  HC_HIP(hipGetLastError());
  return HC_OK;
}
#ifdef HC_IBM_PHASE_TIMES
extern "C" int hc_debug_phase_times(double *out) {
  unsigned long long h[32];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof(h)) != hipSuccess) return HC_ERR_HIP;
  for (int k = 0; k < 32; k++) out[k] = (double)h[k];
  std::memset(h, 0, sizeof(h));
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), h, sizeof(h)) != hipSuccess) return HC_ERR_HIP;
  return HC_OK;
}
#endif

extern "C" {

int hcp_spread(hc_cells *C, int force_limit) {
  HC_REQUIRE(C, "hcp_spread: null pointer");
  int rc = sync_to_device(C); if (rc != HC_OK) return rc;
  if (C->nverts == 0) return HC_OK;
  hc::ProfScope prof(hc::PK_SPREAD);
  if (reproducible()) return spread_reproducible(C, force_limit);
  const LatView v = make_view(C->L);
  for (int t = 0; t < C->ntypes; t++) {
    const long n = C->ncells[t] * C->types[t]->host.nv;
    if (n == 0) continue;
    const int nv = C->types[t]->host.nv;
    if (ibm_width(C, t) != HC_IBM_PHI2) { if ((rc = wide_spread(C, t, force_limit, g_ibm_per_vertex)) != HC_OK) return rc; continue; }
    const TypeArrays a = vert_arrays(C, t);   // r is set exactly when rep_on(), see vert_arrays: the sync_to_device above has run
    if (g_ibm_per_vertex)
      hipLaunchKernelGGL(ibm_spread_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, n, a.p[0], a.p[1], a.p[2], a.f[0], a.f[1], a.f[2],
                         a.r[0], a.r[1], a.r[2], C->L->force[C->L->fcur], force_limit, C->P.f_limit, a.vert_cell, a.tag_all, a.dead);
    else
      hipLaunchKernelGGL(ibm_spread_cell_kernel, dim3((unsigned)C->ncells[t]), dim3(nv > 128 ? 256 : 128), 0, hc::stream(), v, nv, a.p[0], a.p[1], a.p[2],
                         a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2], C->L->force[C->L->fcur], force_limit, C->P.f_limit, 1, a.tag, a.dead);
    HC_HIP(hipGetLastError());
  }
  return HC_OK;
}

int hcp_interpolate(hc_cells *C) {
  HC_REQUIRE(C, "hcp_interpolate: null pointer");
  int rc = sync_to_device(C); if (rc != HC_OK) return rc;
  if (C->nverts == 0) return HC_OK;
  hc::ProfScope prof(hc::PK_INTERP);
  const hc_lattice *L = C->L;
  const LatView v = make_view(L);
  const PopView pv = make_pops(L);
  for (int t = 0; t < C->ntypes; t++) {
    const long n = C->ncells[t] * C->types[t]->host.nv;
    if (n == 0) continue;
    const int nv = C->types[t]->host.nv;
    if (ibm_width(C, t) != HC_IBM_PHI2) { if ((rc = wide_interpolate(C, t, nullptr, 0, g_ibm_per_vertex)) != HC_OK) return rc; continue; }
    const TypeArrays a = vert_arrays(C, t);
    if (g_ibm_per_vertex)
      HC_LAUNCH_POPS(ibm_interpolate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), v, pv, n, a.p[0], a.p[1], a.p[2], a.v[0], a.v[1], a.v[2],
                     a.vert_cell, a.tag_all, a.dead);
    else
      HC_LAUNCH_POPS(ibm_interpolate_cell_kernel, dim3((unsigned)C->ncells[t]), dim3(nv > 128 ? 256 : 128), v, pv, nv, a.p[0], a.p[1], a.p[2], a.v[0], a.v[1], a.v[2],
                     (const int *)nullptr, 1, a.tag, a.dead);
    HC_HIP(hipGetLastError());
  }
  return HC_OK;
}

// the message of a velocity update (slab.hip): u = j/rho + F/2 on this slab's face plane `side`, post-stream state, packed as
// [3][ny*nz] for the neighbour on that side.  The face plane and the plane behind it have been collided and the halo plane
// in front of it holds the neighbour's crossing populations.  A lattice with open-boundary nodes runs the OPEN instantiation,
// like the interpolation kernels (launch_open).
int hcl_face_velocity_pack(hc_lattice *L, int side, double *dev_buf) {
  HC_REQUIRE(L && dev_buf && (side == 0 || side == 1), "hcl_face_velocity_pack: bad arguments");
  LatView v = make_view(L);
  v.halo_u[0] = v.halo_u[1] = nullptr;   // own planes only: nothing here reads a halo velocity
  const PopView pv = make_pops(L);
  HC_LAUNCH_POPS(face_velocity_kernel, dim3((unsigned)((L->plane + 255) / 256), 1, 1), dim3(256), v, pv, side == 0 ? 0 : L->nx - 1, dev_buf, 0, (double *)nullptr);
  HC_HIP(hipGetLastError());
  return HC_OK;
}
// both face planes in one launch (either buffer may be null)
int hcl_face_velocity_pack_both(hc_lattice *L, double *dev_lo, double *dev_hi) {
  HC_REQUIRE(L, "hcl_face_velocity_pack_both: null lattice");
  if (!dev_lo && !dev_hi) return HC_OK;
  if (!dev_lo || !dev_hi) return hcl_face_velocity_pack(L, dev_lo ? 0 : 1, dev_lo ? dev_lo : dev_hi);
  LatView v = make_view(L);
  v.halo_u[0] = v.halo_u[1] = nullptr;
  const PopView pv = make_pops(L);
  HC_LAUNCH_POPS(face_velocity_kernel, dim3((unsigned)((L->plane + 255) / 256), 2, 1), dim3(256), v, pv, 0, dev_lo, L->nx - 1, dev_hi);
  HC_HIP(hipGetLastError());
  return HC_OK;
}

// inspection: the same plane of velocities on the host, [3][ny*nz] (tests; the message itself never touches the host)
int hcl_download_face_velocity(hc_lattice *L, int side, double *host_u) {
  HC_REQUIRE(L && host_u && (side == 0 || side == 1), "hcl_download_face_velocity: bad arguments");
  hc::DevBuf<double> d;
  int rc = d.reserve(3 * L->plane); if (rc != HC_OK) return rc;
  rc = hcl_face_velocity_pack(L, side, d);
  if (rc == HC_OK && hipMemcpyAsync(host_u, d, 3 * L->plane * sizeof(double), hipMemcpyDeviceToHost, hc::stream()) != hipSuccess) { hc::set_error("hcl_download_face_velocity: copy failed"); rc = HC_ERR_HIP; }
  if (rc == HC_OK && hipStreamSynchronize(hc::stream()) != hipSuccess) { hc::set_error("hcl_download_face_velocity: synchronise failed"); rc = HC_ERR_HIP; }
  return rc;
}

int hcp_interpolate_cells(hc_cells *C, int type, const int *slots, int n) { return hcc::interpolate_cells_staged(C, type, slots, n, 1); }

}  // extern "C"

// which: the staging slot the list travels through (a caller that issues several lists in one step gives each its own, so that
// staging the next one does not wait for the copy of the previous one, which may sit behind a whole collide in the stream)
int hcc::interpolate_cells_staged(hc_cells *C, int type, const int *slots, int n, int which) {
  HC_REQUIRE(C && type >= 0 && type < C->ntypes && n >= 0 && which >= 0 && which < 19, "hcp_interpolate_cells: bad arguments");
  if (n == 0) return HC_OK;
  HC_REQUIRE(slots, "hcp_interpolate_cells: null pointer");
  int rc = sync_to_device(C); if (rc != HC_OK) return rc;
  for (int i = 0; i < n; i++) HC_REQUIRE(slots[i] >= 0 && slots[i] < C->ncells[type], "hcp_interpolate_cells: slot out of range");
  int *d_slots = nullptr;
  rc = stage_ints(C, which, &d_slots, slots, n); if (rc != HC_OK) return rc;
  hc::ProfScope prof(hc::PK_INTERP);
  if (ibm_width(C, type) != HC_IBM_PHI2) return wide_interpolate(C, type, d_slots, n, 0);
  const hc_lattice *L = C->L;
  const LatView v = make_view(L);
  const PopView pv = make_pops(L);
  const TypeArrays a = vert_arrays(C, type);
  const int nv = C->types[type]->host.nv;
  HC_LAUNCH_POPS(ibm_interpolate_cell_kernel, dim3((unsigned)n), dim3(nv > 128 ? 256 : 128), v, pv, nv, a.p[0], a.p[1], a.p[2], a.v[0], a.v[1], a.v[2],
                 (const int *)d_slots, 0, a.tag, a.dead);
  HC_HIP(hipGetLastError());
  return HC_OK;
}
