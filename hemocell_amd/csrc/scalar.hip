// The CEPAC field: a passive scalar (a dissolved agonist concentration) on a D3Q19 advection-diffusion lattice bound to one
// hc_lattice, which carries it with the flow's velocity.
//
// Replaces the MultiBlockLattice3D<T, AdvectionDiffusionD3Q19Descriptor> of core/hemoCellFields.cpp:120-133 with its
// AdvectionDiffusionBGKdynamics and the coupling processor that hands it the flow velocity.  The reference leaves the field
// half finished (param::tau_CEPAC is 0 and is passed where an omega belongs) and its fluid library is not part of the reference
// tree, so the step is defined here and pinned by tests/scalar_ref.py, which restates it operation for operation; DESIGN.md
// section 6 lists the deviations.
//
// Layout (HBM): the lattice's own.  Two population buffers g[q][x+HALO][y][z] with the lattice's padded strides (xs, qs), in
// the pull scheme of lattice.hip: the stored state is POST-COLLISION in the shifted representation g_i - t_i, a step gathers
// S(x, i) = P(x - c_i, i), relaxes and writes.  Concentration: C = 1 + sum_i g_i.
//
// One step (scalar_collide_stream_kernel) on a node that is not inert (mask != 2), in this order:
//   1. fluid nodes (mask == 0): the advecting velocity, what the reference's coupling processor would read after
//      collideAndStream of the same iteration.  The flow's 19 post-stream populations are gathered in ascending q and added as
//      they arrive to rhoBar, j_x, j_y, j_z (the order of moments() in d3q19.h); invRho = 1 / (1 + rhoBar);
//      b = the body force (that of the last region holding the node, else the uniform one); F = the IBM force the flow's last
//      collide consumed (0 where the node's dirty group was not touched); u_d = j_d * invRho + (b_d + F_d) / 2.
//   2. the 19 g are gathered (pull).
//   3. wall node (mask != 0): opposite pairs are swapped (full-way bounce-back: zero scalar flux; no Ladd term, whatever the
//      wall's class).
//      source node (class byte k > 0, value C_s = src_val[k - 1]): Cbar = C_s - 1, C = C_s,
//        g_q = t_q * (Cbar + (3 * C) * (c_q . u)) for every q.
//      any other fluid node: Cbar = ((g_0 + g_1) + g_2) + ... + g_18, C = 1 + Cbar, and for every q
//        geq = t_q * (Cbar + (3 * C) * (c_q . u)); g_q = g_q * (1 - omega); g_q = g_q + omega * geq.
//      c_q . u is cdot() of d3q19.h: ((c_x u_x + c_y u_y) + c_z u_z) with the zero terms dropped, 0 for q = 0.
//   4. non-temporal stores of the 19 g.
// The library is built with -ffp-contract=off, so every operation above rounds once.
#include "cells.h"
#include <memory>

struct hc_scalar {
  hc_lattice *L = nullptr;     // not owned; hcl_destroy of a lattice that still has its scalar destroys the scalar first
  double omega = 1.0;
  hc::DevBuf<double> g[2];     // [19][qstride] post-collision populations, ping-pong like hc_lattice::f
  int cur = 0;                 // g[cur] is read by the next step
  hc::DevBuf<uint8_t> src;     // [npad] source class of every node: 0 = none, k = src_val[k - 1]
  std::vector<uint8_t> hsrc;   // host copy, device numbering
  int nsrc = 0; double src_val[HC_MAX_SCALAR_SOURCES];
};

namespace {

struct ScalArgs {
  const double *gin; double *gout;
  const double *fin;       // the flow's populations of the state after hcl_step_end
  const double *F;         // the IBM force the flow's last collide consumed [npad][3]
  const uint8_t *dirty; uint8_t epoch; int ibm;
  const uint8_t *mask, *src;
  int nx, ny, nz, plane; long xs, qs;
  int x_begin, wrap_x, per_y, per_z;
  double omega, bx, by, bz;
  const int *row_z0, *row_cum, *blk_row; int nblk;
  int x0; BodyRegions reg;
  double src_val[HC_MAX_SCALAR_SOURCES];
};

__device__ __forceinline__ Nbr neighbours(const ScalArgs &a, int x, int y, int z) { return hc::neighbours(a, a.xs, x, y, z); }

// step 1 of the file comment on a fluid node
__device__ __forceinline__ void advecting_velocity(const ScalArgs &a, const Nbr &n, int x, int y, int z, long node, double &u0, double &u1, double &u2) {
  double r = 0.0, jx = 0.0, jy = 0.0, jz = 0.0;
#define M(Q, CX, CY, CZ)                                                  \
  {                                                                       \
    bool ok; const long off = src_off<CX, CY, CZ>(n, ok);                 \
    const double fq = ok ? a.fin[(long)Q * a.qs + node + off] : 0.0;      \
    r += fq;                                                              \
    if (CX == 1) jx += fq; else if (CX == -1) jx += -fq;                  \
    if (CY == 1) jy += fq; else if (CY == -1) jy += -fq;                  \
    if (CZ == 1) jz += fq; else if (CZ == -1) jz += -fq;                  \
  }
  FOR_Q(M)
#undef M
  const double invRho = 1.0 / (1.0 + r);
  double bx = a.bx, by = a.by, bz = a.bz;
  if (a.reg.n) region_force(a.reg, a.x0 + x, y, z, bx, by, bz);
  double F0 = 0.0, F1 = 0.0, F2 = 0.0;
  if (a.ibm && a.dirty[node >> 4] == a.epoch) { F0 = a.F[3 * node]; F1 = a.F[3 * node + 1]; F2 = a.F[3 * node + 2]; }
  u0 = jx * invRho + (bx + F0) / 2.0; u1 = jy * invRho + (by + F1) / 2.0; u2 = jz * invRho + (bz + F2) / 2.0;
}

// the value of the node's source class: a chain of selects over the kernel arguments, no indexed access, no scratch
__device__ __forceinline__ double source_value(const ScalArgs &a, uint8_t cls) {
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < HC_MAX_SCALAR_SOURCES; k++) v = cls == k + 1 ? a.src_val[k] : v;
  return v;
}

// the collide's thread -> node mapping through the active-span map (lattice.hip)
__device__ __forceinline__ bool active_node(const ScalArgs &a, int &x, int &y, int &z) {
  x = a.x_begin + (int)blockIdx.y;
  const int xp = x + HALO;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int *cum = a.row_cum + (long)xp * (a.ny + 1);
  if (t >= cum[a.ny]) return false;
  int lo = a.blk_row[(long)xp * (a.nblk + 1) + blockIdx.x], hi = a.blk_row[(long)xp * (a.nblk + 1) + blockIdx.x + 1];
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cum[mid] <= t) lo = mid; else hi = mid - 1; }
  y = lo; z = a.row_z0[(long)xp * a.ny + y] + (t - cum[y]);
  return true;
}

__global__ __launch_bounds__(256) void scalar_collide_stream_kernel(ScalArgs a) {
  int x, y, z;
  if (!active_node(a, x, y, z)) return;
  const long node = (long)(x + HALO) * a.xs + y * a.nz + z;
  const uint8_t m = a.mask[node];
  if (m == 2) return;   // inert solid: nothing reaches it, nothing leaves it
  const uint8_t cls = a.src[node];
  const Nbr n = neighbours(a, x, y, z);
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  if (m == 0) advecting_velocity(a, n, x, y, z, node, u0, u1, u2);   // the flow's populations are summed as they arrive: none stays live beside the g
  double g[HC_Q];
  pull(a.gin, a.qs, node, n, g);
  if (m != 0) {
#pragma unroll
    for (int i = 1; i <= 9; i++) { const double t = g[i]; g[i] = g[i + 9]; g[i + 9] = t; }
  } else {
    double Cbar = 0.0;
#pragma unroll
    for (int q = 0; q < HC_Q; q++) Cbar += g[q];
    double C = 1.0 + Cbar;
    if (cls) { C = source_value(a, cls); Cbar = C - 1.0; }
    const double C3 = 3.0 * C;
    const double one_m_omega = 1.0 - a.omega;
#define M(Q, CX, CY, CZ)                                           \
    {                                                              \
      const double c_u = cdot<CX, CY, CZ>(u0, u1, u2);             \
      const double geq = tq(Q) * (Cbar + C3 * c_u);                \
      double r = g[Q] * one_m_omega;                               \
      r += a.omega * geq;                                          \
      g[Q] = cls ? geq : r;                                        \
    }
    FOR_Q(M)
#undef M
  }
#pragma unroll
  for (int q = 0; q < HC_Q; q++) __builtin_nontemporal_store(g[q], &a.gout[(long)q * a.qs + node]);
}

// ---- everything below is off the step path: one thread per bulk node of a plane, as the observers of lattice.hip
#define HC_PLANE_NODE(a)                                            \
  const int p = blockIdx.x * 256 + threadIdx.x;                     \
  if (p >= a.plane) return;                                         \
  const int x = a.x_begin + blockIdx.y;                             \
  const int y = p / a.nz, z = p - y * a.nz;                         \
  const long node = (long)(x + HALO) * a.xs + p;                    \
  const Nbr n = neighbours(a, x, y, z)

// initializeAtEquilibrium at u = 0 on the nodes of the box (inside the lattice): the box's nodes get their VISIBLE populations,
// so the stored slot P(y, i) is written where its reader y + c_i lies in the box, with the neighbour-mask rule of
// init_eq_kernel: mask[y + c_i] ? 0 : t_i Cbar.  Slots read from outside the box, or by nobody, stay as they are.
__global__ void scalar_init_eq_kernel(ScalArgs a, double Cbar, int bx0, int bx1, int by0, int by1, int bz0, int bz1) {
  HC_PLANE_NODE(a);
#define M(Q, CX, CY, CZ)                                           \
  {                                                                \
    bool ok; const long off = dst_off<CX, CY, CZ>(n, ok);          \
    int tx = x + CX, ty = y + CY, tz = z + CZ;                     \
    if (a.wrap_x) tx = tx < 0 ? a.nx - 1 : tx == a.nx ? 0 : tx;    \
    if (a.per_y) ty = ty < 0 ? a.ny - 1 : ty == a.ny ? 0 : ty;     \
    if (a.per_z) tz = tz < 0 ? a.nz - 1 : tz == a.nz ? 0 : tz;     \
    if (ok && tx >= bx0 && tx <= bx1 && ty >= by0 && ty <= by1 && tz >= bz0 && tz <= bz1) \
      a.gout[(long)Q * a.qs + node] = a.mask[node + off] == 0 ? tq(Q) * Cbar : 0.0; \
  }
  FOR_Q(M)
#undef M
}

// what an observer sees on a node: C_s on a fluid source node, else 1 + the sum of the gathered populations in ascending q
__device__ __forceinline__ double concentration_at(const ScalArgs &a, const Nbr &n, long node) {
  const uint8_t cls = a.src[node];
  if (cls && a.mask[node] == 0) return source_value(a, cls);
  double g[HC_Q];
  pull(a.gin, a.qs, node, n, g);
  double Cbar = 0.0;
#pragma unroll
  for (int q = 0; q < HC_Q; q++) Cbar += g[q];
  return 1.0 + Cbar;
}

__global__ void scalar_concentration_kernel(ScalArgs a, double *out) {
  HC_PLANE_NODE(a);
  out[(long)x * a.plane + p] = concentration_at(a, n, node);
}

// AoS [node][19] of the post-stream state, and its inverse (download_kernel / upload_kernel of lattice.hip for one slab)
__global__ void scalar_download_kernel(ScalArgs a, double *aos) {
  HC_PLANE_NODE(a);
  double g[HC_Q];
  pull(a.gin, a.qs, node, n, g);
  const long o = ((long)x * a.plane + p) * HC_Q;
#pragma unroll
  for (int q = 0; q < HC_Q; q++) aos[o + q] = g[q];
}

__global__ void scalar_upload_kernel(ScalArgs a, const double *aos) {
  HC_PLANE_NODE(a);
  const long bulk = (long)x * a.plane + p;
  Nbr nl = n;   // offsets in the unpadded [x][y][z] numbering of the host array
  nl.xm = nl.xm / a.xs * a.plane; nl.xp = nl.xp / a.xs * a.plane;
#define M(Q, CX, CY, CZ)                                                                  \
  {                                                                                       \
    bool ok; const long off = dst_off<CX, CY, CZ>(nl, ok);                                \
    if (!a.wrap_x && ((CX == 1 && x == a.nx - 1) || (CX == -1 && x == 0))) ok = false;   \
    a.gout[(long)Q * a.qs + node] = ok ? aos[(bulk + off) * HC_Q + Q] : 0.0;             \
  }
  FOR_Q(M)
#undef M
}

// the advecting velocity the next step would use: [node][3], 0 on nodes that are not fluid
__global__ void scalar_velocity_kernel(ScalArgs a, double *u) {
  HC_PLANE_NODE(a);
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  if (a.mask[node] == 0) advecting_velocity(a, n, x, y, z, node, u0, u1, u2);
  const long o = 3 * ((long)x * a.plane + p);
  u[o] = u0; u[o + 1] = u1; u[o + 2] = u2;
}

// sum, minimum and maximum of C over the fluid nodes (the fixed-grid reduction of common.h)
__global__ __launch_bounds__(256) void scalar_stats_kernel(ScalArgs a, double *partial) {
  StatAcc acc{1e300, -1e300, 0.0, 0};
  const long nbulk = (long)a.nx * a.plane;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nbulk; k += (long)STAT_BLOCKS * 256) {
    const int x = (int)(k / a.plane), p = (int)(k - (long)x * a.plane);
    const long node = (long)(x + HALO) * a.xs + p;
    if (a.mask[node] != 0) continue;
    const int y = p / a.nz, z = p - y * a.nz;
    stat_add(acc, concentration_at(a, neighbours(a, x, y, z), node));
  }
  stat_block_store(acc, partial);
}

// C at the vertices: the IBM interpolation's stencil (phi2_stencil: fluid nodes only, weights renormalised) applied to the
// concentration, out = sum_k w_k C(node_k) in ascending stencil order.  One thread per vertex of one cell type; removed
// vertices and vertices of cells that are gone give 0.
__global__ __launch_bounds__(256) void scalar_sample_kernel(LatView v, ScalArgs a, long nvert, const double *px, const double *py, const double *pz,
                                                            const int *vert_cell, const int *tag, const unsigned char *dead, double *out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvert) return;
  if (dead[i] || tag[vert_cell[i]] == 1) { out[i] = 0.0; return; }
  Stencil s;
  phi2_stencil(v, px[i], py[i], pz[i], s);
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (s.node[k] < 0) continue;
    c += concentration_at(a, neighbours(a, s.lx[k], s.ly[k], s.lz[k]), s.node[k]) * s.w[k];
  }
  out[i] = c;
}

// the arguments for the state after hcl_step_end: g[cur] and f[cur] hold what was last written, force[(fcur + 2) % 3] the force
// the flow's last collide consumed, with the dirty map and epoch it was spread under.  It stays intact until the next collide
// zeroes it, and the spread of the next iteration adds to force[fcur]: a step beside that spread reads nothing it writes.
ScalArgs make_args(const hc_scalar *S) {
  const hc_lattice *L = S->L;
  ScalArgs a;
  a.gin = S->g[S->cur]; a.gout = S->g[1 - S->cur];
  a.fin = L->f[L->cur];
  const int fused = (L->fcur + 2) % 3;
  a.F = L->force[fused]; a.dirty = L->fdirty[fused]; a.epoch = L->fepoch[fused]; a.ibm = L->ibm;
  a.mask = L->mask; a.src = S->src;
  a.nx = L->nx; a.ny = L->ny; a.nz = L->nz; a.plane = (int)L->plane; a.xs = (long)L->xs; a.qs = (long)L->qstride;
  a.x_begin = 0; a.wrap_x = L->periodic[0]; a.per_y = L->periodic[1]; a.per_z = L->periodic[2];   // n_slabs == 1
  a.omega = S->omega; a.bx = L->body[0]; a.by = L->body[1]; a.bz = L->body[2];
  a.row_z0 = L->row_z0; a.row_cum = L->row_cum; a.blk_row = L->blk_row; a.nblk = L->nblk;
  a.x0 = L->x0; a.reg = L->regions;
  for (int k = 0; k < HC_MAX_SCALAR_SOURCES; k++) a.src_val[k] = k < S->nsrc ? S->src_val[k] : 0.0;
  return a;
}

dim3 plane_grid(const hc_lattice *L) { return dim3((unsigned)((L->plane + 255) / 256), (unsigned)L->nx, 1); }

int upload_sources(hc_scalar *S) {
  HC_HIP(hipMemcpyAsync(S->src, S->hsrc.data(), S->L->npad, hipMemcpyHostToDevice, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

// per_node doubles for every bulk node, written by launch(scratch) and copied to the host (download() of lattice.hip)
template <class Launch>
int download(hc_scalar *S, double *dst, size_t per_node, Launch launch) {
  hc_lattice *L = S->L;
  const size_t n = (size_t)L->nx * L->plane * per_node;
  const int rc = L->scratch.reserve(n); if (rc != HC_OK) return rc;
  launch((double *)L->scratch);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(dst, L->scratch, n * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

}  // namespace

void hc::scalar_lattice_destroyed(hc_lattice *L) { if (L->scalar) hcl_scalar_destroy(L->scalar); }

extern "C" {

int hcl_scalar_create(hc_lattice *L, double omega, hc_scalar **out) {
  HC_REQUIRE(L && out, "hcl_scalar_create: null pointer");
  HC_REQUIRE(omega > 0.0 && omega < 2.0, "hcl_scalar_create: omega must be in (0,2)");
  HC_REQUIRE(L->n_slabs == 1, "hcl_scalar_create: the scalar field needs the whole domain on one GPU (n_slabs = 1)");
  HC_REQUIRE(L->ob_n == 0, "hcl_scalar_create: the lattice has open-boundary nodes; the scalar field and open boundaries do not combine");
  HC_REQUIRE(!L->le_on, "hcl_scalar_create: the lattice has a Lees-Edwards boundary; the scalar field and Lees-Edwards do not combine");
  HC_REQUIRE(L->visc_n == 0, "hcl_scalar_create: the lattice has interior viscosity enabled; the scalar field and interior viscosity do not combine");
  HC_REQUIRE(!hc::in_preinlet_pair(L), "hcl_scalar_create: the lattice is part of a pre-inlet pair; the scalar field and a pre-inlet do not combine");
  HC_REQUIRE(!L->scalar, "hcl_scalar_create: the lattice has a scalar field already (one per lattice)");
  std::unique_ptr<hc_scalar> S(new hc_scalar());
  S->L = L; S->omega = omega;
  int rc;
  for (int k = 0; k < 2; k++) {
    if ((rc = S->g[k].reserve(L->qstride * HC_Q)) != HC_OK) return rc;
    HC_HIP(hipMemsetAsync(S->g[k], 0, L->qstride * HC_Q * sizeof(double), hc::stream()));   // C = 1 everywhere
  }
  if ((rc = S->src.reserve(L->npad)) != HC_OK) return rc;
  HC_HIP(hipMemsetAsync(S->src, 0, L->npad, hc::stream()));
  S->hsrc.assign(L->npad, 0);
  HC_HIP(hipStreamSynchronize(hc::stream()));
  L->scalar = S.get();
  *out = S.release();
  return HC_OK;
}

int hcl_scalar_destroy(hc_scalar *S) {
  if (!S) return HC_OK;
  hipStreamSynchronize(hc::stream());
  S->L->scalar = nullptr;
  delete S;
  return HC_OK;
}

int hcl_scalar_init_equilibrium(hc_scalar *S, const int box[6], double C) {
  HC_REQUIRE(S, "hcl_scalar_init_equilibrium: null pointer");
  const hc_lattice *L = S->L;
  const int whole[6] = {0, L->nx - 1, 0, L->ny - 1, 0, L->nz - 1};
  const int *b = box ? box : whole;
  HC_REQUIRE(b[0] <= b[1] && b[2] <= b[3] && b[4] <= b[5], "hcl_scalar_init_equilibrium: empty box");
  ScalArgs a = make_args(S);
  a.gout = S->g[S->cur];
  // the part of the box inside the lattice (the kernel reads the mask of nodes in the box only)
  hipLaunchKernelGGL(scalar_init_eq_kernel, plane_grid(L), dim3(256), 0, hc::stream(), a, C - 1.0, std::max(b[0], whole[0]), std::min(b[1], whole[1]),
                     std::max(b[2], whole[2]), std::min(b[3], whole[3]), std::max(b[4], whole[4]), std::min(b[5], whole[5]));
  HC_HIP(hipGetLastError());
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

// The value table holds the values in use: a value whose nodes have all been painted over gives its slot back here, so the
// limit counts the distinct values on the lattice after the call.  A refused call changes nothing; a box that holds no node of
// the lattice registers nothing.
int hcl_scalar_set_source_box(hc_scalar *S, const int box[6], double C) {
  HC_REQUIRE(S && box, "hcl_scalar_set_source_box: null pointer");
  HC_REQUIRE(box[0] <= box[1] && box[2] <= box[3] && box[4] <= box[5], "hcl_scalar_set_source_box: empty box");
  HC_REQUIRE(C == C, "hcl_scalar_set_source_box: the value is not a number");
  const hc_lattice *L = S->L;
  const int b[6] = {std::max(box[0], 0), std::min(box[1], L->nx - 1), std::max(box[2], 0), std::min(box[3], L->ny - 1), std::max(box[4], 0), std::min(box[5], L->nz - 1)};
  if (b[0] > b[1] || b[2] > b[3] || b[4] > b[5]) return HC_OK;   // wholly outside the lattice
  auto paint = [&](std::vector<uint8_t> &cls, uint8_t v) {
    for (int x = b[0]; x <= b[1]; x++)
      for (int y = b[2]; y <= b[3]; y++)
        for (int z = b[4]; z <= b[5]; z++) cls[(size_t)(x + HALO) * L->xs + (size_t)y * L->nz + z] = v;
  };
  std::vector<uint8_t> cls(S->hsrc);
  paint(cls, 0);
  bool used[HC_MAX_SCALAR_SOURCES + 1] = {false};
  for (const uint8_t c : cls) used[c] = true;
  uint8_t renumber[HC_MAX_SCALAR_SOURCES + 1] = {0};
  double val[HC_MAX_SCALAR_SOURCES]; int n = 0;
  for (int k = 0; k < S->nsrc; k++) if (used[k + 1]) { val[n] = S->src_val[k]; renumber[k + 1] = (uint8_t)++n; }
  int k = 0;
  while (k < n && val[k] != C) k++;
  HC_REQUIRE(k < HC_MAX_SCALAR_SOURCES, "hcl_scalar_set_source_box: more than HC_MAX_SCALAR_SOURCES distinct source values");
  if (k == n) val[n++] = C;
  for (uint8_t &c : cls) c = renumber[c];
  paint(cls, (uint8_t)(k + 1));
  S->hsrc.swap(cls); S->nsrc = n;
  for (int i = 0; i < n; i++) S->src_val[i] = val[i];
  return upload_sources(S);
}

int hcl_scalar_clear_sources(hc_scalar *S) {
  HC_REQUIRE(S, "hcl_scalar_clear_sources: null pointer");
  std::fill(S->hsrc.begin(), S->hsrc.end(), 0);
  S->nsrc = 0;
  return upload_sources(S);
}

int hcl_scalar_step(hc_scalar *S) {
  HC_REQUIRE(S, "hcl_scalar_step: null pointer");
  const hc_lattice *L = S->L;
  hc::ProfScope prof(hc::PK_SCALAR);
  hipLaunchKernelGGL(scalar_collide_stream_kernel, dim3((unsigned)((L->max_active + 255) / 256), (unsigned)L->nx, 1), dim3(256), 0, hc::stream(), make_args(S));
  HC_HIP(hipGetLastError());
  S->cur ^= 1;
  return HC_OK;
}

int hcl_scalar_download(hc_scalar *S, double *C_out) {
  HC_REQUIRE(S && C_out, "hcl_scalar_download: null pointer");
  return download(S, C_out, 1, [&](double *out) { hipLaunchKernelGGL(scalar_concentration_kernel, plane_grid(S->L), dim3(256), 0, hc::stream(), make_args(S), out); });
}

int hcl_scalar_download_populations(hc_scalar *S, double *g_aos) {
  HC_REQUIRE(S && g_aos, "hcl_scalar_download_populations: null pointer");
  return download(S, g_aos, HC_Q, [&](double *out) { hipLaunchKernelGGL(scalar_download_kernel, plane_grid(S->L), dim3(256), 0, hc::stream(), make_args(S), out); });
}

int hcl_scalar_upload_populations(hc_scalar *S, const double *g_aos) {
  HC_REQUIRE(S && g_aos, "hcl_scalar_upload_populations: null pointer");
  hc_lattice *L = S->L;
  const size_t nd = (size_t)L->nx * L->plane * HC_Q;
  const int rc = L->scratch.reserve(nd); if (rc != HC_OK) return rc;
  HC_HIP(hipMemcpyAsync(L->scratch, g_aos, nd * sizeof(double), hipMemcpyHostToDevice, hc::stream()));
  ScalArgs a = make_args(S);
  a.gout = S->g[S->cur];
  hipLaunchKernelGGL(scalar_upload_kernel, plane_grid(L), dim3(256), 0, hc::stream(), a, (const double *)L->scratch);
  HC_HIP(hipGetLastError());
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcl_scalar_download_velocity(hc_scalar *S, double *u_out) {
  HC_REQUIRE(S && u_out, "hcl_scalar_download_velocity: null pointer");
  return download(S, u_out, 3, [&](double *out) { hipLaunchKernelGGL(scalar_velocity_kernel, plane_grid(S->L), dim3(256), 0, hc::stream(), make_args(S), out); });
}

int hcl_scalar_stats(hc_scalar *S, double out[3]) {
  HC_REQUIRE(S && out, "hcl_scalar_stats: null pointer");
  hc_lattice *L = S->L;
  const int rc = L->scratch.reserve((size_t)STAT_BLOCKS * 4); if (rc != HC_OK) return rc;
  hipLaunchKernelGGL(scalar_stats_kernel, dim3(STAT_BLOCKS), dim3(256), 0, hc::stream(), make_args(S), (double *)L->scratch);
  HC_HIP(hipGetLastError());
  double mms[3]; long n;
  const int rc2 = hc::stat_finish(L->scratch, mms, &n); if (rc2 != HC_OK) return rc2;
  out[0] = mms[2]; out[1] = mms[0]; out[2] = mms[1];   // sum, minimum, maximum
  return HC_OK;
}

int hcp_sample_scalar(hc_cells *C, hc_scalar *S, double *out_per_vertex) {
  HC_REQUIRE(C && S && out_per_vertex, "hcp_sample_scalar: null pointer");
  HC_REQUIRE(C->L == S->L, "hcp_sample_scalar: the cells and the scalar field are bound to different lattices");
  HC_REQUIRE(!C->ibm_wide_on(), "hcp_sample_scalar: a cell type is on a three- or four-point IBM kernel; the sample goes through the eight-node stencil");
  int rc = settle(C); if (rc != HC_OK) return rc;
  if ((rc = sync_to_device(C)) != HC_OK) return rc;
  if (C->nverts == 0) return HC_OK;
  if ((rc = C->info.d.reserve((size_t)C->nverts)) != HC_OK) return rc;
  const LatView v = make_view(C->L);
  const ScalArgs a = make_args(S);
  long o = 0;   // vertices in download order: type by type, a type's cells side by side
  for (int t = 0; t < C->ntypes; t++) {
    const long n = C->ncells[t] * C->types[t]->host.nv;
    if (n == 0) continue;
    const TypeArrays va = vert_arrays(C, t);
    hipLaunchKernelGGL(scalar_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, a, n, (const double *)va.p[0], (const double *)va.p[1],
                       (const double *)va.p[2], va.vert_cell, (const int *)va.tag_all, (const unsigned char *)va.dead, C->info.d + o);
    HC_HIP(hipGetLastError());
    o += n;
  }
  HC_HIP(hipMemcpyAsync(out_per_vertex, C->info.d, (size_t)o * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

}  // extern "C"
