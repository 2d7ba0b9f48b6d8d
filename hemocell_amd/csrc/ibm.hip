// Immersed-boundary coupling on the GPU: force spreading and velocity interpolation with the two-point delta function of the
// reference and the three-point (Roma) and four-point (Peskin) ones of hcp_type_set_ibm_kernel.  Every kernel is written once
// over the stencil policy of a width (ibm_common.h: Phi<W>).
//
// Replaces (file:line in the HemoCell tree):
//   core/immersedBoundaryMethod.h:62-138          interpolationCoefficientsPhi2 (cells.h: phi2_stencil)
//   core/hemoCellParticleField.cpp:841-863        spreadParticleForce
//   core/hemoCellParticleField.cpp:819-839        interpolateFluidVelocity
//
// Three forms: one thread per vertex (hc_debug_ibm_per_vertex), one workgroup per cell on an LDS tile (the default), and the
// entries of the reproducible spread (hc_set_reproducible_spread).
#include "ibm_common.h"
#include <hipcub/hipcub.hpp>
#include <cstdlib>
#include <numeric>

namespace {

// FORCE_LIMIT cap, core/hemoCellParticleField.cpp:848-852 (mutates sv.force: the caller stores a force that was scaled)
__device__ __forceinline__ bool cap_force(double f[3], double f_limit) {
  const double mag = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
  if (mag > f_limit) {
    const double sc = f_limit / mag;
    f[0] *= sc; f[1] *= sc; f[2] *= sc;
    return true;
  }
  return false;
}

// force_repulsion + force (:857-859); the repulsion arrays are null while no repulsion is on
__device__ __forceinline__ void driving_force(const double *rx, const double *ry, const double *rz, long i, const double f[3], double g[3]) {
  g[0] = (rx ? rx[i] : 0.0) + f[0]; g[1] = (ry ? ry[i] : 0.0) + f[1]; g[2] = (rz ? rz[i] : 0.0) + f[2];
}

// external.data[d] += (force_repulsion[d] + force[d]) * weight  (:857-859) with global atomics; g = force_repulsion + force
__device__ __forceinline__ void add_to_node(const LatView &v, double *F, long node, const double g[3], double w) {
  v.dirty[node >> 4] = v.epoch;
  double *Fn = F + 3 * node;
  unsafeAtomicAdd(Fn, g[0] * w); unsafeAtomicAdd(Fn + 1, g[1] * w); unsafeAtomicAdd(Fn + 2, g[2] * w);
}

// one vertex with its own gathers: u = sum over the admitted nodes, in visiting order, of u(node) * weight
template <class S, bool OPEN>
__device__ __forceinline__ void interpolate_vertex(const LatView &v, const Pops<OPEN> &pv, double px, double py, double pz, double out[3]) {
  typename S::Global s; typename S::Axes ax;
  S::stencil(v, px, py, pz, s, ax);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  S::for_each(v, s, ax, [&](int, bool adm, long node, int lx, int ly, int lz, double w) __attribute__((always_inline)) {
    if (!adm) return;
    double u[3];
    node_velocity<OPEN>(v, pv, lx, ly, lz, node, u);
    a0 += (u[0] * w); a1 += (u[1] * w); a2 += (u[2] * w);
  });
  out[0] = a0; out[1] = a1; out[2] = a2;
}

// ----------------------------------------------------------------------------
// one thread per vertex
template <class S>
__global__ __launch_bounds__(256) void ibm_spread_kernel(LatView v, long n, const double *px, const double *py, const double *pz,
                                                         double *fx, double *fy, double *fz, const double *rx, const double *ry, const double *rz,
                                                         double *F, int limit_on, double f_limit, const int *vert_cell, const int *tag, const unsigned char *dead) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag[vert_cell[i]] == 1) return;   // removed particle / cell gone
  double f[3] = {fx[i], fy[i], fz[i]};
  if (limit_on && cap_force(f, f_limit)) { fx[i] = f[0]; fy[i] = f[1]; fz[i] = f[2]; }
  typename S::Global s; typename S::Axes ax;
  S::stencil(v, px[i], py[i], pz[i], s, ax);
  double g[3];
  driving_force(rx, ry, rz, i, f, g);
  S::for_each(v, s, ax, [&](int, bool adm, long node, int, int, int, double w) __attribute__((always_inline)) { if (adm) add_to_node(v, F, node, g, w); });
}

template <class S, bool OPEN>
__global__ __launch_bounds__(256) void ibm_interpolate_kernel(LatView v, Pops<OPEN> pv, long n, const double *px, const double *py,
                                                              const double *pz, double *vx, double *vy, double *vz, const int *vert_cell, const int *tag,
                                                              const unsigned char *dead) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag[vert_cell[i]] == 1) return;
  double u[3];
  interpolate_vertex<S, OPEN>(v, pv, px[i], py[i], pz[i], u);
  vx[i] = u[0]; vy[i] = u[1]; vz[i] = u[2];
}

// ----------------------------------------------------------------------------
// reproducible spread (hc_set_reproducible_spread).  The reference adds particle by particle in storage order
// (core/hemoCellParticleField.cpp:841-863), so a node's force is a sum in a fixed order and a run repeats bit for bit; the
// atomic kernels add in whatever order the hardware takes them.  Here every (particle, stencil node) becomes an entry keyed by
// its node, written in the canonical order (cell type, cell id, vertex id, stencil node): W^3 per vertex from entry ebase on,
// a node that is not admitted with an invalid key.  A stable radix sort by node groups the entries of a node without
// disturbing that order, and ONE thread per node sums them in sequence and adds the sum to the node.  The order does not
// depend on the storage slots of the cells, so every slab that holds a node forms the bits the single domain forms.
template <class S>
__global__ __launch_bounds__(256) void spread_emit_kernel(LatView v, int nv, long n, const int *order, long ebase, const double *px, const double *py,
                                                          const double *pz, double *fx, double *fy, double *fz, const double *rx, const double *ry,
                                                          const double *rz, int limit_on, double f_limit, const int *tag, const unsigned char *dead,
                                                          unsigned int *keys, int *vals, double *c0, double *c1, double *c2) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;   // (rank of the cell in id order) * nv + vertex
  if (g >= n) return;
  const int cell = order[g / nv];
  const long i = (long)cell * nv + (g % nv);
  const long e0 = ebase + g * (S::W * S::W * S::W);
  const bool live = tag[cell] != 1 && !dead[i];   // removed particle / cell gone: its entries stay empty
  typename S::Global s; typename S::Axes ax;
  S::none(s);
  double f[3] = {0.0, 0.0, 0.0};
  if (live) {
    f[0] = fx[i]; f[1] = fy[i]; f[2] = fz[i];
    if (limit_on && cap_force(f, f_limit)) { fx[i] = f[0]; fy[i] = f[1]; fz[i] = f[2]; }
    if (rx) { f[0] = rx[i] + f[0]; f[1] = ry[i] + f[1]; f[2] = rz[i] + f[2]; }   // force_repulsion + force, :857-859
    S::stencil(v, px[i], py[i], pz[i], s, ax);
  }
  S::for_each(v, s, ax, [&](int k, bool adm, long node, int, int, int, double w) __attribute__((always_inline)) {
    keys[e0 + k] = adm ? (unsigned int)node : 0xffffffffu;
    vals[e0 + k] = (int)(e0 + k);
    c0[e0 + k] = adm ? f[0] * w : 0.0; c1[e0 + k] = adm ? f[1] * w : 0.0; c2[e0 + k] = adm ? f[2] * w : 0.0;
  });
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


// ----------------------------------------------------------------------------
// LDS-tiled IBM kernels: one workgroup per cell.
//
// All stencils of a cell fall into the cell's bounding box; the nodes the cell touches are compacted into a list
// (compact_nodes).  Spread: the workgroup accumulates the three force components per listed node in LDS (ds_add_f64), then
// flushes them to HBM with one fp64 atomic per (node, component) -- several times fewer, better shaped global atomics than one
// per (vertex, node, component).  Interpolate: the node velocity (19-population gather + moments) is evaluated once per listed
// node into LDS, and every vertex then blends its W^3 values from LDS.
// LDS of both (ibm_common.h: the caps): 16-bit slots, and the node list reuses the mask tile (the mask is only read while the
// stencils are formed).

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

// shared prologue of the two cell kernels: positions -> registers, tile, mask tile (two points: only near walls), admission.
// returns false (uniformly) when the cell does not fit the tile and the caller must take the per-vertex path
// dead: removed particles of an INCOMPLETE cell (null for a complete one); they take no part in anything
template <class S>
__device__ __forceinline__ bool cell_prologue(const LatView &v, int nv, long base, const double *px, const double *py, const double *pz,
                                              const unsigned char *dead, int *s_red, unsigned char *mt, Tile &t, typename S::Kept vs[NVPT]) {
  const int tid = threadIdx.x, nth = blockDim.x;
  double p[NVPT][3]; int b[NVPT][3]; bool live[NVPT];
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    const int i = tid + j * nth;
    live[j] = i < nv && !(dead && dead[base + i]);
    if (live[j]) {
      p[j][0] = px[base + i]; p[j][1] = py[base + i]; p[j][2] = pz[base + i];
      S::rows(p[j], b[j], vs[j]);
#pragma unroll
      for (int a = 0; a < 3; a++) { lo[a] = min(lo[a], b[j][a]); hi[a] = max(hi[a], b[j][a] + S::W - 1); }
    }
  }
  block_bbox(lo, hi, s_red, t);
  if (!tile_finish(v, t, S::TILE) || nv > NVPT * nth) return false;
  bool clear = false;
  if constexpr (S::WALL_BRICKS) clear = tile_is_clear(v, t);   // uniform
  if (!clear) {
#pragma unroll 4
    for (int i = tid; i < t.vol; i += nth) mt[i] = tile_mask(v, t, i);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    vs[j].adm = 0; vs[j].base = 0;
    if (live[j]) S::admit(t, clear ? nullptr : mt, p[j], b[j], vs[j]);
  }
  return true;
}

// the FORCE_LIMIT cap of a cell's vertices: those a thread holds in registers (f), else strided over the stored forces
__device__ __forceinline__ void cap_cell_forces(int nv, long base, double *fx, double *fy, double *fz, const unsigned char *dead, double f_limit,
                                                bool in_regs, double f[NVPT][3]) {
  const int tid = threadIdx.x, nth = blockDim.x;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < NVPT; j++) {
      const int i = tid + j * nth;
      if (i < nv && !(dead && dead[base + i]) && cap_force(f[j], f_limit)) {   // a removed particle is not in the list: its force stays
        fx[base + i] = f[j][0]; fy[base + i] = f[j][1]; fz[base + i] = f[j][2];
      }
    }
  } else {
    for (int i = tid; i < nv; i += nth) {
      if (dead && dead[base + i]) continue;
      double g[3] = {fx[base + i], fy[base + i], fz[base + i]};
      if (cap_force(g, f_limit)) { fx[base + i] = g[0]; fy[base + i] = g[1]; fz[base + i] = g[2]; }
    }
  }
}

// per-vertex spread with direct global atomics: cells larger than the tile or touching more than S::NODES nodes
template <class S>
__device__ void spread_direct(const LatView &v, int nv, long base, const double *px, const double *py, const double *pz, const double *fx,
                              const double *fy, const double *fz, const double *rx, const double *ry, const double *rz, double *F,
                              const unsigned char *dead) {
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    if (dead && dead[base + i]) continue;
    typename S::Global s; typename S::Axes ax;
    S::stencil(v, px[base + i], py[base + i], pz[base + i], s, ax);
    const double f[3] = {fx[base + i], fy[base + i], fz[base + i]};
    double g[3];
    driving_force(rx, ry, rz, base + i, f, g);
    S::for_each(v, s, ax, [&](int, bool adm, long node, int, int, int, double w) __attribute__((always_inline)) { if (adm) add_to_node(v, F, node, g, w); });
  }
}

template <class S>
__global__ __launch_bounds__(256) void ibm_spread_cell_kernel(LatView v, int nv, const double *px, const double *py, const double *pz,
                                                              double *fx, double *fy, double *fz, const double *rx, const double *ry, const double *rz,
                                                              double *F, int limit_on, double f_limit, int xcd_ranges, const int *tag, const unsigned char *vdead) {
  // the three force components of a touched node side by side (acc[3 * rank + component], the layout of F)
  __shared__ unsigned short slot[S::TILE];
  __shared__ __attribute__((aligned(16))) unsigned char raw[S::TILE > 2 * S::NODES ? S::TILE : 2 * S::NODES];
  unsigned char *mt = raw; unsigned short *list = reinterpret_cast<unsigned short *>(raw);
  __shared__ double acc[3 * S::NODES];
  __shared__ int s_red[6 * MAXW], s_count;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int cell = xcd_ranges ? xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
  const int state = tag[cell];
  if (state == 1) return;                                        // the cell is gone
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
  Tile t; typename S::Kept vs[NVPT];
  const bool tiled = cell_prologue<S>(v, nv, base, px, py, pz, dead, s_red, mt, t, vs);
  if (limit_on) cap_cell_forces(nv, base, fx, fy, fz, dead, f_limit, in_regs, f);
  // The touched nodes are compacted and all three components accumulated per node in LDS (ds_add_f64), then flushed with one
  // fp64 atomic per (node, component), consecutive lanes on consecutive addresses: a z-run of a membrane across a row leaves as
  // one 48-96 byte segment of F instead of three 16-32 byte segments in three component planes.
  const int n = tiled ? compact_nodes<S>(t, vs, slot, list, &s_count) : 0;
  if (!tiled || n > S::NODES) { spread_direct<S>(v, nv, base, px, py, pz, fx, fy, fz, rx, ry, rz, F, dead); return; }   // uniform
  const int sy = t.e[2], sx = t.e[1] * t.e[2];
  for (int k = tid; k < 3 * n; k += nth) acc[k] = 0.0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NVPT; j++) {
    const int i = tid + j * nth;
    if (i >= nv || !vs[j].adm) continue;
    double g[3];
    driving_force(rx, ry, rz, base + i, f[j], g);
    S::for_each(vs[j], sx, sy, [&](int at, double w) __attribute__((always_inline)) {
      double *a = &acc[3 * slot[at]];
      atomicAdd(a, g[0] * w); atomicAdd(a + 1, g[1] * w); atomicAdd(a + 2, g[2] * w);
    });
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

template <class S, bool OPEN>
__global__ __launch_bounds__(256) void ibm_interpolate_cell_kernel(LatView v, Pops<OPEN> pv, int nv, const double *px, const double *py,
                                                                   const double *pz, double *vx, double *vy, double *vz, const int *slots, int xcd_ranges,
                                                                   const int *tag, const unsigned char *vdead) {
  __shared__ unsigned short slot[S::TILE];
  __shared__ __attribute__((aligned(16))) unsigned char raw[S::TILE > 2 * S::NODES ? S::TILE : 2 * S::NODES];
  unsigned char *mt = raw; unsigned short *list = reinterpret_cast<unsigned short *>(raw);
  __shared__ double ux[S::NODES], uy[S::NODES], uz[S::NODES];
  __shared__ int s_red[6 * MAXW], s_count;
  const int tid = threadIdx.x, nth = blockDim.x;
  const int cell = slots ? slots[blockIdx.x] : (xcd_ranges ? xcd_contiguous((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x);   // slots: only the listed cells of the type
  const int state = tag[cell];
  if (state == 1) return;
  const unsigned char *dead = state == 2 ? vdead : nullptr;
  const long base = (long)cell * nv;
  Tile t; typename S::Kept vs[NVPT];
  bool tiled = cell_prologue<S>(v, nv, base, px, py, pz, dead, s_red, mt, t, vs);
  if (tiled && compact_nodes<S>(t, vs, slot, list, &s_count) > S::NODES) tiled = false;   // uniform: s_count is shared
  if (tiled) {
    const int sy = t.e[2], sx = t.e[1] * t.e[2];
    const int n = s_count;
    for (int k = tid; k < n; k += nth) {       // node velocity once per node
      int lx, ly, lz;
      const long node = tile_node(v, t, list[k], lx, ly, lz);
      double u[3];
      node_velocity<OPEN>(v, pv, lx, ly, lz, node, u);
      ux[k] = u[0]; uy[k] = u[1]; uz[k] = u[2];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NVPT; j++) {
      const int i = tid + j * nth;
      if (i >= nv || (dead && dead[base + i])) continue;   // a removed particle keeps its velocity, as in the per-vertex forms
      double a0 = 0.0, a1 = 0.0, a2 = 0.0;
      S::for_each(vs[j], sx, sy, [&](int at, double w) __attribute__((always_inline)) {
        const int q = slot[at];
        a0 += (ux[q] * w); a1 += (uy[q] * w); a2 += (uz[q] * w);
      });
      vx[base + i] = a0; vy[base + i] = a1; vz[base + i] = a2;
    }
    return;
  }
  for (int i = tid; i < nv; i += nth) {   // fallback: per-vertex gathers
    if (dead && dead[base + i]) continue;
    double u[3];
    interpolate_vertex<S, OPEN>(v, pv, px[base + i], py[base + i], pz[base + i], u);
    vx[base + i] = u[0]; vy[base + i] = u[1]; vz[base + i] = u[2];
  }
}

// The policy of a stencil width (ibm_width): f(Phi<W>{}), in the style of hc::launch_open
template <class F>
void with_width(int w, F f) {
  if (w == HC_IBM_PHI3) f(Phi<3>{});
  else if (w == HC_IBM_PHI4) f(Phi<4>{});
  else f(Phi<2>{});
}
// hc::launch_open for a kernel K<S, OPEN>: the OPEN instantiations exist for two points only (a three- or four-point kernel is
// refused on a lattice with open boundaries, and its four-point interpolation has no registers left for one)
template <class S, class Launch>
void launch_pops(const hc_lattice *L, const PopView &pv, Launch launch) {
  if constexpr (S::W == 2) hc::launch_open(L, pv, launch);
  else launch(std::false_type{}, pv);
}
// threads of a per-cell workgroup: NVPT vertices per thread cover the largest mesh
dim3 cell_block(int nv) { return dim3(nv > 128 ? 256 : 128); }

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
  // entries: W^3 per vertex of a type.  A type's entries start on a multiple of 8; entries in between keep an invalid key
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
    const TypeArrays a = vert_arrays(C, t);   // r is set exactly when rep_on(), see vert_arrays: hcp_spread has synchronised to the device
    with_width(ibm_width(C, t), [&](auto s) {
      hipLaunchKernelGGL(spread_emit_kernel<decltype(s)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, nv, n,
                         (const int *)(d_order + obase[(size_t)t]), first_e[t], a.p[0], a.p[1], a.p[2], a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2], force_limit,
                         C->P.f_limit, a.tag, a.dead, C->det_keys[0], C->det_vals[0], C->det_val[0], C->det_val[1], C->det_val[2]);
    });
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

// the interpolation of one type.  d_slots: device list of n_slots cell slots, or null for every cell of the type (then
// hc_debug_ibm_per_vertex picks the per-vertex form)
static int interpolate_type(hc_cells *C, int t, const int *d_slots, int n_slots) {
  const hc_lattice *L = C->L;
  const int w = ibm_width(C, t);
  HC_REQUIRE(w == HC_IBM_PHI2 || (L->ob_n == 0 && L->n_slabs == 1), "hcp_interpolate: a three- or four-point IBM kernel on a lattice with open boundaries or slabs");   // refused at set-up, both ways
  const LatView v = make_view(L);
  const PopView pv = make_pops(L);
  const int nv = C->types[t]->host.nv;
  const long n = C->ncells[t] * nv;
  const TypeArrays a = vert_arrays(C, t);
  with_width(w, [&](auto s) {
    using S = decltype(s);
    launch_pops<S>(L, pv, [&](auto open, const auto &pops) {
      constexpr bool OPEN = decltype(open)::value;
      if (g_ibm_per_vertex && !d_slots)
        hipLaunchKernelGGL((ibm_interpolate_kernel<S, OPEN>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, pops, n, a.p[0], a.p[1], a.p[2],
                           a.v[0], a.v[1], a.v[2], a.vert_cell, a.tag_all, a.dead);
      else   // XCD-contiguous cell order: the full launch on two points (untried on three and four)
        hipLaunchKernelGGL((ibm_interpolate_cell_kernel<S, OPEN>), dim3(d_slots ? (unsigned)n_slots : (unsigned)C->ncells[t]), cell_block(nv), 0, hc::stream(), v, pops,
                           nv, a.p[0], a.p[1], a.p[2], a.v[0], a.v[1], a.v[2], d_slots, !d_slots && S::W == 2, a.tag, a.dead);
    });
  });
  HC_HIP(hipGetLastError());
  return HC_OK;
}

extern "C" {

int hcp_spread(hc_cells *C, int force_limit) {
  HC_REQUIRE(C, "hcp_spread: null pointer");
  int rc = sync_to_device(C); if (rc != HC_OK) return rc;
  if (C->nverts == 0) return HC_OK;
  hc::ProfScope prof(hc::PK_SPREAD);
  if (reproducible()) return spread_reproducible(C, force_limit);
  const LatView v = make_view(C->L);
  double *F = C->L->force[C->L->fcur];
  for (int t = 0; t < C->ntypes; t++) {
    const int nv = C->types[t]->host.nv;
    const long n = C->ncells[t] * nv;
    if (n == 0) continue;
    const TypeArrays a = vert_arrays(C, t);   // r is set exactly when rep_on(), see vert_arrays: the sync_to_device above has run
    with_width(ibm_width(C, t), [&](auto s) {
      using S = decltype(s);
      if (g_ibm_per_vertex)
        hipLaunchKernelGGL(ibm_spread_kernel<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, n, a.p[0], a.p[1], a.p[2], a.f[0], a.f[1], a.f[2],
                           a.r[0], a.r[1], a.r[2], F, force_limit, C->P.f_limit, a.vert_cell, a.tag_all, a.dead);
      else
        hipLaunchKernelGGL(ibm_spread_cell_kernel<S>, dim3((unsigned)C->ncells[t]), cell_block(nv), 0, hc::stream(), v, nv, a.p[0], a.p[1], a.p[2],
                           a.f[0], a.f[1], a.f[2], a.r[0], a.r[1], a.r[2], F, force_limit, C->P.f_limit, S::W == 2, a.tag, a.dead);
    });
    HC_HIP(hipGetLastError());
  }
  return HC_OK;
}

int hcp_interpolate(hc_cells *C) {
  HC_REQUIRE(C, "hcp_interpolate: null pointer");
  int rc = sync_to_device(C); if (rc != HC_OK) return rc;
  if (C->nverts == 0) return HC_OK;
  hc::ProfScope prof(hc::PK_INTERP);
  for (int t = 0; t < C->ntypes; t++)
    if (C->ncells[t] * C->types[t]->host.nv != 0 && (rc = interpolate_type(C, t, nullptr, 0)) != HC_OK) return rc;
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

// the width of a type's delta function.  The lattice-side registry (hc::ibm_wide) lets open boundaries and the pre-inlet refuse
// a lattice that has a type on three or four points
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
  return interpolate_type(C, type, d_slots, n);
}
