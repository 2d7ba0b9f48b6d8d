// D3Q19 Guo-forced BGK collide-stream for gfx950.
//
// Replaces Palabos MultiBlockLattice3D::collideAndStream() as called from
// HemoCell::iterate (core/hemoCell.cpp:317) with GuoExternalForceBGKdynamics
// (examples/pipeflow/pipeflow.cpp:71) and BounceBack walls (:73), plus the two
// setExternalVector sweeps of core/hemoCell.cpp:369-371 and
// examples/pipeflow/pipeflow.cpp:144-146 (fused: the body force is a kernel
// argument, the per-node IBM force buffer of the *other* parity is zeroed here).
//
// Layout (HBM): structure of arrays f[q][x+HALO][y][z], z fastest, so that a
// wavefront reads/writes 64 consecutive doubles of one population and an
// x-plane of one population is contiguous (halo pack = plain copies).  Two
// population buffers (A/B "pull" scheme): the stored state is the
// POST-COLLISION field P_t; a step gathers S_t(x,i) = P_{t-1}(x - c_i, i)
// (misaligned reads, aligned writes), collides and writes P_t.  The reference's
// visible state after collideAndStream (post-stream S) is recovered by
// hcl_download_populations with the same gather.
//
// Arithmetic follows oracle/hemo_oracle.c operation for operation (the library
// is built with -ffp-contract=off) so that fluid-only runs are bit-identical.
#include "common.h"
#include "comm.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <type_traits>

using namespace hc;

namespace {

struct LatArgs {
  const double *fin;
  double *fout;
  const double *Fin;   // IBM force to read   [npad][3]
  double *Fzero;       // IBM force to zero   [npad][3]
  const uint8_t *mask;
  int nx, ny, nz;
  int plane;             // nodes of one x-plane
  long xs;               // elements from x-plane to x-plane (plane + padding)
  long npad;
  long qs;               // population stride (npad + padding)
  int x_begin;
  int x_split, x_jump;   // one launch over two ranges of planes (the planes next to the two faces of a slab): blockIdx.y >= x_split -> x += x_jump
  int wrap_x, per_y, per_z;
  double omega;
  double bx, by, bz;
  const int *row_z0, *row_cum, *blk_row;
  int nblk;
  int ibm;               // 0: no membrane cells are bound to this lattice -> the IBM force buffers are not touched
  const uint8_t *dirty_in, *dirty_zero; uint8_t epoch_in, epoch_zero;
  double wall_u[4][3];   // moving-wall classes 3..6
  int x0, nx_global;     // global x of plane 0 (body-force regions are given in global coordinates)
  BodyRegions reg;
};

// the arguments of the open-boundary instantiation: the other instantiations keep LatArgs, and with it their kernel-argument block
struct OpenArgs : LatArgs {
  const int *ob_code;    // Zou-He open boundaries: -1 or axis << 29 | slot << 2 | kind
  const double *ob_val;  // [slot][4] {u_x, u_y, u_z, rho}
};
template <bool OPEN> using Args = std::conditional_t<OPEN, OpenArgs, LatArgs>;

// the arguments of the interior-viscosity instantiation of the collide (launch_collide picks it while visc_n > 0), by the same
// rule: the class byte of every node and the omegas of the classes 1 .. HC_MAX_VISC_CLASSES
struct ViscArgs : LatArgs {
  const uint8_t *visc_class;               // [npad]: 0 = the lattice's omega, k = omega_class[k - 1]
  double omega_class[HC_MAX_VISC_CLASSES];
};
template <bool OPEN, bool VISC> using CollideArgs = std::conditional_t<VISC, ViscArgs, Args<OPEN>>;

// uniform body force, or that of the last region holding the node
__device__ __forceinline__ void body_at(const LatArgs &a, int x, int y, int z, double &bx, double &by, double &bz) {
  bx = a.bx; by = a.by; bz = a.bz;
  if (a.reg.n) region_force(a.reg, a.x0 + x, y, z, bx, by, bz);
}

// the gather's neighbour and wrap rules (d3q19.h) on the arguments of this file's kernels
__device__ __forceinline__ Nbr neighbours(const LatArgs &a, int x, int y, int z) { return hc::neighbours(a, a.xs, x, y, z); }

// What an observer sees on a node: the gathered populations f -- on an open lattice those of a fluid Zou-He node completed as the
// collide is about to complete them, so that a velocity node reports u_bc (+ F / 2) and a pressure node its prescribed density
// instead of moments that count the unknown populations as the zeros that came from outside -- and their moments.
struct Moments { double rhoBar, j0, j1, j2, invRho; };
template <bool OPEN>
__device__ __forceinline__ Moments observe(const Args<OPEN> &a, int x, int y, int z, long node, double f[HC_Q]) {
  pull(a.fin, a.qs, node, neighbours(a, x, y, z), f);
  if constexpr (OPEN) {
    if (a.mask[node] == 0) {
      const int code = a.ob_code[node];
      if (code >= 0) zou_he_node(f, code, a.ob_val);
    }
  }
  Moments m;
  moments(f, m.rhoBar, m.j0, m.j1, m.j2);
  m.invRho = 1.0 / (1.0 + m.rhoBar);
  return m;
}

// GuoExternalForceBGKdynamics::collide, operation order of oracle/hemo_oracle.c collide_guo_bgk
__device__ __forceinline__ void collide_guo(double f[HC_Q], double Fx, double Fy, double Fz, double omega) {
  double rhoBar, j0, j1, j2;
  moments(f, rhoBar, j0, j1, j2);
  const double invRho = 1.0 / (1.0 + rhoBar);
  const double rho = 1.0 + rhoBar;
  const double u0 = j0 * invRho + Fx / 2.0, u1 = j1 * invRho + Fy / 2.0, u2 = j2 * invRho + Fz / 2.0;
  j0 = rho * u0; j1 = rho * u1; j2 = rho * u2;
  const double jSqr = j0 * j0 + j1 * j1 + j2 * j2;
  const double one_m_omega = 1.0 - omega;
  const double guo = 1.0 - omega / 2.0;
#define M(Q, CX, CY, CZ)                                                                     \
  {                                                                                          \
    const double c_j = cdot<CX, CY, CZ>(j0, j1, j2);                                         \
    const double feq = tq(Q) * (rhoBar + 3.0 * c_j + invRho * (4.5 * c_j * c_j - 1.5 * jSqr)); \
    f[Q] *= one_m_omega;                                                                     \
    f[Q] += omega * feq;                                                                     \
  }
  FOR_Q(M)
#undef M
#define M(Q, CX, CY, CZ)                                                                     \
  {                                                                                          \
    double c_u = cdot<CX, CY, CZ>(u0, u1, u2);                                               \
    c_u *= 9.0;                                                                              \
    double ft = (((double)CX - u0) * 3.0 + c_u * (double)CX) * Fx;                           \
    ft += (((double)CY - u1) * 3.0 + c_u * (double)CY) * Fy;                                 \
    ft += (((double)CZ - u2) * 3.0 + c_u * (double)CZ) * Fz;                                 \
    ft *= tq(Q);                                                                             \
    ft *= guo;                                                                               \
    f[Q] += ft;                                                                              \
  }
  FOR_Q(M)
#undef M
}

// OPEN: the instantiation for lattices with Zou-He nodes (launch_collide picks it while ob_n > 0); the other instantiations
// compile to the same code as before it existed.  VISC: the instantiation for lattices with interior viscosity
// (hcl_interior_enable), under the same rule; it differs in the omega a fluid node relaxes with and in nothing else.  The two
// never combine (hcl_interior_enable and the open-boundary calls refuse each other).
template <bool REGIONS, bool OPEN = false, bool VISC = false>
__global__ __launch_bounds__(256) void collide_stream_kernel(CollideArgs<OPEN, VISC> a) {
  static_assert(!(OPEN && VISC), "open boundaries and interior viscosity do not share a lattice");
  // thread -> (y,z) through the active-span map of this plane: consecutive threads walk the spans of
  // consecutive rows, so every lane of every wave (except the last of a plane) has a live node
  const int x = a.x_begin + (int)blockIdx.y + ((int)blockIdx.y >= a.x_split ? a.x_jump : 0);
  const int xp = x + HALO;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int *cum = a.row_cum + (long)xp * (a.ny + 1);
  if (t >= cum[a.ny]) return;
  int lo = a.blk_row[(long)xp * (a.nblk + 1) + blockIdx.x], hi = a.blk_row[(long)xp * (a.nblk + 1) + blockIdx.x + 1];
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cum[mid] <= t) lo = mid; else hi = mid - 1; }
  const int y = lo, z = a.row_z0[(long)xp * a.ny + y] + (t - cum[y]);
  const int p = y * a.nz + z;
  const long node = (long)(x + HALO) * a.xs + p;
  const uint8_t m = a.mask[node];
  uint8_t vclass = 0;   // the class byte travels with the mask byte
  if constexpr (VISC) vclass = a.visc_class[node];
  if (m == 2) return;   // solid node with no fluid neighbour: inert under full-way bounce-back
  const Nbr n = neighbours(a, x, y, z);
  // the node's IBM force record (24 B) is loaded together with the populations, in one round trip.  This also keeps the
  // kernel at 98 VGPRs, 4 waves per SIMD: loaded after the pull it compiles to 94 VGPRs and 5 waves, and the spread's
  // waves beside it then wait for two collide waves to retire (spread 0.72 instead of 0.33 ms)
  const bool fdirty = a.ibm && m == 0 && a.dirty_in[node >> 4] == a.epoch_in;
  double F0 = 0.0, F1 = 0.0, F2 = 0.0;
  if (fdirty) { F0 = a.Fin[3 * node]; F1 = a.Fin[3 * node + 1]; F2 = a.Fin[3 * node + 2]; }
  double f[HC_Q];
  pull(a.fin, a.qs, node, n, f);
  const bool wall = m != 0;
  if (wall) {
    // BounceBack::collide: swap opposite pairs (full-way bounce-back)
#pragma unroll
    for (int i = 1; i <= 9; i++) { double t = f[i]; f[i] = f[i + 9]; f[i + 9] = t; }
    if (m >= 3) {
      // moving no-slip wall: Ladd's momentum term at rho = 1, f_opp(i) = f_i - 6 t_i (c_i.u_w); after the
      // swap slot o holds f_i, so the term of direction i = opp(o) is subtracted from slot o
      const double w0 = a.wall_u[m - 3][0], w1 = a.wall_u[m - 3][1], w2 = a.wall_u[m - 3][2];
#define M(Q, CX, CY, CZ)                                                                  \
      if (Q != 0) {                                                                       \
        constexpr int O = Q <= 9 ? Q + 9 : Q - 9;                                         \
        const double c_u = (double)CX * w0 + (double)CY * w1 + (double)CZ * w2;           \
        f[O] = f[O] - 6.0 * tq(Q) * c_u;                                                  \
      }
      FOR_Q(M)
#undef M
    }
  } else {
    double bx = a.bx, by = a.by, bz = a.bz;
    if (REGIONS) region_force(a.reg, a.x0 + x, y, z, bx, by, bz);
    double Fx = bx, Fy = by, Fz = bz;
    if (fdirty) {   // x + 0.0 == x, so skipping untouched groups changes no bits
      Fx = bx + F0; Fy = by + F1; Fz = bz + F2;
    }
    if constexpr (OPEN) {
      const int code = a.ob_code[node];
      if (code >= 0) zou_he_node(f, code, a.ob_val);
    }
    double omega = a.omega;
    if constexpr (VISC) {   // a chain of selects over the kernel arguments: no indexed access, no scratch
#pragma unroll
      for (int k = 0; k < HC_MAX_VISC_CLASSES; k++) omega = vclass == k + 1 ? a.omega_class[k] : omega;
    }
    collide_guo(f, Fx, Fy, Fz, omega);
  }
#pragma unroll
  // streamed once and read again only after 5 GB of other traffic: non-temporal stores keep the lines out of the way
  // of the loads (measured: -3 % kernel time on the pipe and on the all-fluid box; non-temporal loads cost 4 %)
  for (int q = 0; q < HC_Q; q++) __builtin_nontemporal_store(f[q], &a.fout[(long)q * a.qs + node]);
  if (a.ibm && a.dirty_zero[node >> 4] == a.epoch_zero) { a.Fzero[3 * node] = 0.0; a.Fzero[3 * node + 1] = 0.0; a.Fzero[3 * node + 2] = 0.0; }
}

// P(y,i) = mask[y+c_i] ? 0 : feq_i(rho,u): initializeAtEquilibrium in the shifted representation
__global__ void init_eq_kernel(LatArgs a, double rhoBar, double j0, double j1, double j2) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const int y = p / a.nz, z = p - y * a.nz;
  const long node = (long)(x + HALO) * a.xs + p;
  const Nbr n = neighbours(a, x, y, z);
  const double invRho = 1.0 / (1.0 + rhoBar);
  const double jSqr = j0 * j0 + j1 * j1 + j2 * j2;
#define M(Q, CX, CY, CZ)                                                                        \
  {                                                                                             \
    bool ok; long off = dst_off<CX, CY, CZ>(n, ok);                                             \
    double v = 0.0;                                                                             \
    if (ok && a.mask[node + off] == 0) {                                                        \
      const double c_j = cdot<CX, CY, CZ>(j0, j1, j2);                                          \
      v = tq(Q) * (rhoBar + 3.0 * c_j + invRho * (4.5 * c_j * c_j - 1.5 * jSqr));               \
    }                                                                                           \
    a.fout[(long)Q * a.qs + node] = v;                                                          \
  }
  FOR_Q(M)
#undef M
}

// AoS [node][19] of the post-stream state, bulk nodes only
__global__ void download_kernel(LatArgs a, double *aos) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const int y = p / a.nz, z = p - y * a.nz;
  const long node = (long)(x + HALO) * a.xs + p;
  const Nbr n = neighbours(a, x, y, z);
  double f[HC_Q];
  pull(a.fin, a.qs, node, n, f);
  const long o = ((long)x * a.plane + p) * HC_Q;
#pragma unroll
  for (int q = 0; q < HC_Q; q++) aos[o + q] = f[q];
}

// inverse of download: P(y,i) = S(y+c_i, i) (0 if the target lies outside)
// lo_ok / hi_ok: the post-stream state of the plane below / above the slab is in aos as well (planes -1 and nx of the host
// numbering, fetched from the neighbouring ranks)
__global__ void upload_kernel(LatArgs a, const double *aos, int lo_ok, int hi_ok) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const int y = p / a.nz, z = p - y * a.nz;
  const long node = (long)(x + HALO) * a.xs + p;
  const long bulk = (long)x * a.plane + p;
  Nbr nl = neighbours(a, x, y, z);   // offsets in the unpadded [x][y][z] numbering of the host array
  nl.xm = nl.xm / a.xs * a.plane; nl.xp = nl.xp / a.xs * a.plane;
#define M(Q, CX, CY, CZ)                                                                  \
  {                                                                                       \
    bool ok; long off = dst_off<CX, CY, CZ>(nl, ok);                                      \
    /* without x wrap the +-x neighbour of a face plane belongs to the neighbouring rank, or lies outside the domain */ \
    if (!a.wrap_x && ((CX == 1 && x == a.nx - 1 && !hi_ok) || (CX == -1 && x == 0 && !lo_ok))) ok = false; \
    a.fout[(long)Q * a.qs + node] = ok ? aos[(bulk + off) * HC_Q + Q] : 0.0;            \
  }
  FOR_Q(M)
#undef M
}

// What hcl_download_rho_u reports on a node, from the moments observe() took there: rho = 1 + rhoBar and
// u = j / rho + (body + IBM force) / 2 with the IBM force of the buffer the next collide reads.  One function for the download
// kernel and the running statistics (stats_fluid_kernel), so that both form the same bits.
__device__ __forceinline__ void rho_u_values(const LatArgs &a, const Moments &m, int x, int y, int z, long node, double &rho, double u[3]) {
  rho = 1.0 + m.rhoBar;
  double bx, by, bz;
  body_at(a, x, y, z, bx, by, bz);
  u[0] = m.j0 * m.invRho + (bx + a.Fin[3 * node]) / 2.0;
  u[1] = m.j1 * m.invRho + (by + a.Fin[3 * node + 1]) / 2.0;
  u[2] = m.j2 * m.invRho + (bz + a.Fin[3 * node + 2]) / 2.0;
}

// Off-equilibrium part of the momentum-flux tensor, as Palabos' momentTemplates::compute_rhoBar_j_PiNeq forms it from the
// stored populations f_i - t_i: Pi_ab = sum_i c_ia c_ib fbar_i - j_a j_b / rho - cs2 rhoBar delta_ab, components in the
// order xx, xy, xz, yy, yz, zz.  Output fields only (shear stress, strain rate); nothing on the step path reads it.  Shared by
// the download kernel and the running statistics, as rho_u_values is.
__device__ __forceinline__ void pi_neq_values(const double f[HC_Q], const Moments &m, double pi[6]) {
  const double rhoBar = m.rhoBar, j0 = m.j0, j1 = m.j1, j2 = m.j2, invRho = m.invRho;
  double xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
#define M(Q, CX, CY, CZ)                       \
  if (CX * CX) xx += f[Q];                     \
  if (CX * CY == 1) xy += f[Q]; else if (CX * CY == -1) xy += -f[Q]; \
  if (CX * CZ == 1) xz += f[Q]; else if (CX * CZ == -1) xz += -f[Q]; \
  if (CY * CY) yy += f[Q];                     \
  if (CY * CZ == 1) yz += f[Q]; else if (CY * CZ == -1) yz += -f[Q]; \
  if (CZ * CZ) zz += f[Q];
  FOR_Q(M)
#undef M
  const double cs2 = 1.0 / 3.0;
  pi[0] = xx - invRho * j0 * j0 - cs2 * rhoBar;
  pi[1] = xy - invRho * j0 * j1;
  pi[2] = xz - invRho * j0 * j2;
  pi[3] = yy - invRho * j1 * j1 - cs2 * rhoBar;
  pi[4] = yz - invRho * j1 * j2;
  pi[5] = zz - invRho * j2 * j2 - cs2 * rhoBar;
}

template <bool OPEN = false>
__global__ void rho_u_kernel(Args<OPEN> a, double *rho, double *u) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const int y = p / a.nz, z = p - y * a.nz;
  const long node = (long)(x + HALO) * a.xs + p;
  double f[HC_Q];
  const Moments m = observe<OPEN>(a, x, y, z, node, f);
  const long o = (long)x * a.plane + p;
  double r, v[3];
  rho_u_values(a, m, x, y, z, node, r, v);
  rho[o] = r;
  u[3 * o] = v[0]; u[3 * o + 1] = v[1]; u[3 * o + 2] = v[2];
}

template <bool OPEN = false>
__global__ void pi_neq_kernel(Args<OPEN> a, double *pi) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const int y = p / a.nz, z = p - y * a.nz;
  const long node = (long)(x + HALO) * a.xs + p;
  double f[HC_Q];
  const Moments m = observe<OPEN>(a, x, y, z, node, f);
  double v[6];
  pi_neq_values(f, m, v);
  const long o = 6 * ((long)x * a.plane + p);
#pragma unroll
  for (int k = 0; k < 6; k++) pi[o + k] = v[k];
}

// One sample of the running statistics (stats.hip): every selected fluid set takes what the two kernels above report on the
// node, from ONE gather of its populations.  acc holds 16 planes of the node's padded numbering, `stride` doubles apart, in the
// order rho, u (3), uu (6: xx, xy, xz, yy, yz, zz), pi (6); a plane of a set that was not selected is never touched (and not
// allocated).  Consecutive lanes hold consecutive z, so every plane is read and written in whole lines like a population.  One
// thread owns a node and samples are serial on the stream: acc += value in sample order, the host loop's bits.
template <bool OPEN = false>
__global__ __launch_bounds__(256) void stats_fluid_kernel(Args<OPEN> a, int what, double *acc_rho_u, double *acc_uu, double *acc_pi, long stride) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const int y = p / a.nz, z = p - y * a.nz;
  const long node = (long)(x + HALO) * a.xs + p;
  double f[HC_Q];
  const Moments m = observe<OPEN>(a, x, y, z, node, f);
  if (what & (HC_STATS_RHO_U | HC_STATS_UU)) {
    double r, u[3];
    rho_u_values(a, m, x, y, z, node, r, u);
    if (what & HC_STATS_RHO_U) {
      acc_rho_u[node] += r;
#pragma unroll
      for (int d = 0; d < 3; d++) acc_rho_u[(1 + d) * stride + node] += u[d];
    }
    if (what & HC_STATS_UU) {   // the product is rounded, then added (-ffp-contract=off)
      const double uu[6] = {u[0] * u[0], u[0] * u[1], u[0] * u[2], u[1] * u[1], u[1] * u[2], u[2] * u[2]};
#pragma unroll
      for (int k = 0; k < 6; k++) acc_uu[k * stride + node] += uu[k];
    }
  }
  if (what & HC_STATS_PI) {
    double v[6];
    pi_neq_values(f, m, v);
#pragma unroll
    for (int k = 0; k < 6; k++) acc_pi[k * stride + node] += v[k];
  }
}

// Cell::computeVelocity with the body force alone on the listed nodes of the plane coordinate[AXIS] == plane of the lattice `a`:
// out[stride * k .. + 2] = u(node idx[k]).  idx[k] is the node's offset with the axis removed: y * nz + z, x * nz + z,
// x * ny + y for AXIS 0, 1, 2 (x local); on a z plane consecutive nodes lie nz doubles apart, as in the Lees-Edwards layers, but
// a plane is small.  Bounce-back nodes give 0.  hcl_plane_velocity[_axis] writes [n][3]; applyPreInlet on the device
// (hcl_preinlet_apply) writes the velocity components of the domain's slots, [n][4], and leaves rho (component 3) alone.
template <bool OPEN, int AXIS>
__global__ void plane_velocity_kernel(Args<OPEN> a, int plane, const int *idx, int n, double *out, int stride) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int p = idx[k];
  const int x = AXIS == 0 ? plane : AXIS == 1 ? p / a.nz : p / a.ny;
  const int y = AXIS == 0 ? p / a.nz : AXIS == 1 ? plane : p - x * a.ny;
  const int z = AXIS == 0 ? p - y * a.nz : AXIS == 1 ? p - x * a.nz : plane;
  const long node = (long)(x + HALO) * a.xs + (AXIS == 0 ? p : y * a.nz + z);
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  if (a.mask[node] == 0) {
    double f[HC_Q];
    const Moments m = observe<OPEN>(a, x, y, z, node, f);
    double bx, by, bz;
    body_at(a, x, y, z, bx, by, bz);
    u0 = m.j0 * m.invRho + bx / 2.0; u1 = m.j1 * m.invRho + by / 2.0; u2 = m.j2 * m.invRho + bz / 2.0;
  }
  double *o = out + (long)stride * k;
  o[0] = u0; o[1] = u1; o[2] = u2;
}

// ob_val[first + i][c0 .. c0 + nc - 1] = src[i][0 .. nc - 1]
__global__ void ob_set_kernel(double *val, int first, int n, const double *src, int c0, int nc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n * nc) return;
  const int i = k / nc, c = k - i * nc;
  val[4L * (first + i) + c0 + c] = src[k];
}

__global__ void force_aos_kernel(LatArgs a, double *F) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.plane) return;
  const int x = a.x_begin + blockIdx.y;
  const long node = (long)(x + HALO) * a.xs + p;
  const long o = (long)x * a.plane + p;
  for (int d = 0; d < 3; d++) F[3 * o + d] = a.Fin[3 * node + d];
}

// FluidInfo statistics (helper/fluidInfo.cpp:33-96): magnitude of Cell::computeVelocity (what 0) or of the external
// force (what 1) over the non-boundary bulk nodes; what 2: rhoBar = sum of the 19 stored populations, all bulk nodes
template <bool OPEN = false>
__global__ __launch_bounds__(256) void fluid_stats_kernel(Args<OPEN> a, int what, double *partial) {
  StatAcc acc{1e300, -1e300, 0.0, 0};
  const long nbulk = (long)a.nx * a.plane;
  for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < nbulk; k += (long)STAT_BLOCKS * 256) {
    const int x = (int)(k / a.plane), p = (int)(k - (long)x * a.plane);
    const long node = (long)(x + HALO) * a.xs + p;
    if (what == 2) {   // mass: sum of the stored populations of EVERY bulk node (walls park what bounces back)
      double r = 0.0;
#pragma unroll
      for (int q = 0; q < HC_Q; q++) r += a.fin[(long)q * a.qs + node];
      stat_add(acc, r);
      continue;
    }
    if (a.mask[node] != 0) continue;
    const int y = p / a.nz, z = p - y * a.nz;
    double bx, by, bz;
    body_at(a, x, y, z, bx, by, bz);
    double Fx = bx, Fy = by, Fz = bz;
    if (a.ibm) { Fx = bx + a.Fin[3 * node]; Fy = by + a.Fin[3 * node + 1]; Fz = bz + a.Fin[3 * node + 2]; }
    double v0 = Fx, v1 = Fy, v2 = Fz;
    if (what == 0) {
      double f[HC_Q];
      const Moments m = observe<OPEN>(a, x, y, z, node, f);
      v0 = m.j0 * m.invRho + Fx / 2.0; v1 = m.j1 * m.invRho + Fy / 2.0; v2 = m.j2 * m.invRho + Fz / 2.0;
    }
    stat_add(acc, sqrt(v0 * v0 + v1 * v1 + v2 * v2));
  }
  stat_block_store(acc, partial);
}

// ---- Lees-Edwards pass (helper/leesEdwardsBC.h): LeesEdwardsBCGetPopulations / LeesEdwardsBCSetPopulations, the two data
// processors Palabos runs after the stream of collideAndStream().  Only lattices with hcl_set_lees_edwards run it.
// Thread t -> layer t / (nx ny) (0: top z = nz-1, 1: bottom z = 0), x, y.  le_buf is [2][19][nx ny].

// BGKdynamics::collideExternal(cell, rhoBar, j, thetaBar = 0): bgk_ma2 relaxation towards the equilibrium of the given rhoBar
// and j, no forcing term; the operation order of collide_guo's relaxation loop
__device__ __forceinline__ void collide_external(double f[HC_Q], double rhoBar, double j0, double j1, double j2, double omega) {
  const double invRho = 1.0 / (1.0 + rhoBar);
  const double jSqr = j0 * j0 + j1 * j1 + j2 * j2;
  const double one_m_omega = 1.0 - omega;
#define M(Q, CX, CY, CZ)                                                                     \
  {                                                                                          \
    const double c_j = cdot<CX, CY, CZ>(j0, j1, j2);                                         \
    const double feq = tq(Q) * (rhoBar + 3.0 * c_j + invRho * (4.5 * c_j * c_j - 1.5 * jSqr)); \
    f[Q] *= one_m_omega;                                                                     \
    f[Q] += omega * feq;                                                                     \
  }
  FOR_Q(M)
#undef M
}

__device__ __forceinline__ long modp(long a, long b) { return (a % b + b) % b; }

// the Get processor: every value from the state before the pass
__global__ __launch_bounds__(256) void le_gather_kernel(LatArgs a, double *buf, double D, double v_top, double v_bottom) {
  const long nxy = (long)a.nx * a.ny;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * nxy) return;
  const int top = t < nxy ? 1 : 0;
  const long r = top ? t : t - nxy;
  const int x = (int)(r / a.ny), y = (int)(r - (long)x * a.ny);
  const int z = top ? a.nz - 1 : 0;
  const long row = (long)y * a.nz + z;
  const long node = (long)(x + HALO) * a.xs + row;
  double f[HC_Q];
  pull(a.fin, a.qs, node, neighbours(a, x, y, z), f);
  double rhoBar = 0.0;
#pragma unroll
  for (int q = 0; q < HC_Q; q++) rhoBar += f[q];
  collide_external(f, rhoBar, top ? v_top : v_bottom, 0.0, 0.0, a.omega);
  // the two source nodes of the same layer; the fraction g of s1 and (1 - g) of s2 (D < 0: g < 0, an extrapolation)
  const double g = fmod(D, 1.0);
  const long s1 = top ? modp((long)ceil(D + (double)x), a.nx) : modp((long)floor(-D + (double)x), a.nx);
  const long s2 = top ? modp((long)floor(D + (double)x), a.nx) : modp((long)ceil(-D + (double)x), a.nx);
  double f1[HC_Q], f2[HC_Q];   // only the five populations used below are loaded
  pull(a.fin, a.qs, (s1 + HALO) * a.xs + row, neighbours(a, (int)s1, y, z), f1);
  pull(a.fin, a.qs, (s2 + HALO) * a.xs + row, neighbours(a, (int)s2, y, z), f2);
  if (top) {   // 3 <- 3, 6 <- 16, 8 <- 8, 16 <- 6, 18 <- 18
    f[3] = g * f1[3] + (1 - g) * f2[3];
    f[6] = g * f1[16] + (1 - g) * f2[16];
    f[8] = g * f1[8] + (1 - g) * f2[8];
    f[16] = g * f1[6] + (1 - g) * f2[6];
    f[18] = g * f1[18] + (1 - g) * f2[18];
  } else {     // 7 <- 15, 9 <- 9, 12 <- 12, 15 <- 7, 17 <- 17
    f[7] = g * f1[15] + (1 - g) * f2[15];
    f[9] = g * f1[9] + (1 - g) * f2[9];
    f[12] = g * f1[12] + (1 - g) * f2[12];
    f[15] = g * f1[7] + (1 - g) * f2[7];
    f[17] = g * f1[17] + (1 - g) * f2[17];
  }
  double *o = buf + (long)(1 - top) * HC_Q * nxy + r;
#pragma unroll
  for (int q = 0; q < HC_Q; q++) o[(long)q * nxy] = f[q];
}

// the Set processor: S(n, q) is stored in the slot P(n - c_q, q) that pull() reads for node n.  Each slot has exactly one
// reader, so this changes the post-stream state of the two layers and nothing else.
__global__ __launch_bounds__(256) void le_scatter_kernel(LatArgs a, const double *buf) {
  const long nxy = (long)a.nx * a.ny;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * nxy) return;
  const int top = t < nxy ? 1 : 0;
  const long r = top ? t : t - nxy;
  const int x = (int)(r / a.ny), y = (int)(r - (long)x * a.ny);
  const int z = top ? a.nz - 1 : 0;
  const long node = (long)(x + HALO) * a.xs + (long)y * a.nz + z;
  const Nbr n = neighbours(a, x, y, z);
  const double *in = buf + (long)(1 - top) * HC_Q * nxy + r;
#define M(Q, CX, CY, CZ)                                                       \
  {                                                                            \
    bool ok; const long off = src_off<CX, CY, CZ>(n, ok);                      \
    if (ok) a.fout[(long)Q * a.qs + node + off] = in[(long)Q * nxy];           \
  }
  FOR_Q(M)
#undef M
}

struct HaloArgs {
  double *f;          // population buffer
  double *buf;        // contiguous staging
  double *buf2; int n_first;   // entries e >= n_first belong to the second staging block (both faces in one launch)
  long npad; long xs; int plane;   // npad: population stride, xs: x-plane stride
  int n;              // (population, plane) entries
  int pop[HC_Q + 5];  // population of entry e
  int xp[HC_Q + 5];   // padded x index of its plane
  int to_buf;
};
__global__ void halo_copy_kernel(HaloArgs h) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= h.plane) return;
  const int e = blockIdx.y;
  const long li = (long)h.pop[e] * h.npad + (long)h.xp[e] * h.xs + p;
  double *b = e < h.n_first ? h.buf + (long)e * h.plane + p : h.buf2 + (long)(e - h.n_first) * h.plane + p;
  if (h.to_buf) *b = h.f[li]; else h.f[li] = *b;
}

// clears the 2*HALO halo planes of the IBM force (3 doubles per node)
__global__ void zero_force_halo_kernel(double *F, long xs, int plane, int nx) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // (node of the plane, component)
  if (e >= 3 * plane) return;
  const int w = blockIdx.y;
  const int xp = w < HALO ? w : nx + w;   // padded plane index: 0..HALO-1 and nx+HALO..nx+2*HALO-1
  F[3 * (long)xp * xs + e] = 0.0;
}

LatArgs make_args(const hc_lattice *L) {
  LatArgs a;
  a.fin = L->f[L->cur]; a.fout = L->f[1 - L->cur];
  const int fprev = (L->fcur + 2) % 3;
  a.Fin = L->force[L->fcur]; a.Fzero = L->force[fprev];
  a.x_split = 0x7fffffff; a.x_jump = 0;
  a.mask = L->mask;
  a.nx = L->nx; a.ny = L->ny; a.nz = L->nz; a.plane = (int)L->plane; a.xs = (long)L->xs; a.npad = (long)L->npad; a.qs = (long)L->qstride;
  a.x_begin = 0;
  a.wrap_x = (L->n_slabs == 1 && L->periodic[0]) ? 1 : 0;
  a.per_y = L->periodic[1]; a.per_z = L->periodic[2];
  a.omega = L->omega; a.bx = L->body[0]; a.by = L->body[1]; a.bz = L->body[2];
  a.x0 = L->x0; a.nx_global = L->nx_global; a.reg = L->regions;
  a.row_z0 = L->row_z0; a.row_cum = L->row_cum; a.blk_row = L->blk_row; a.nblk = L->nblk;
  a.ibm = L->ibm;
  a.dirty_in = L->fdirty[L->fcur]; a.dirty_zero = L->fdirty[fprev]; a.epoch_in = L->fepoch[L->fcur]; a.epoch_zero = L->fepoch[fprev];
  for (int c = 0; c < 4; c++) for (int d = 0; d < 3; d++) a.wall_u[c][d] = L->wall_u[c][d];
  return a;
}

// the arguments of the open-boundary instantiations (hc::launch_open)
OpenArgs open_of(const hc_lattice *L, const LatArgs &a) {
  OpenArgs o;
  static_cast<LatArgs &>(o) = a;
  o.ob_code = L->ob_code; o.ob_val = L->ob_val;
  return o;
}

// the arguments of the interior-viscosity instantiation of the collide
ViscArgs visc_of(const hc_lattice *L, const LatArgs &a) {
  ViscArgs v;
  static_cast<LatArgs &>(v) = a;
  v.visc_class = L->visc_class;
  for (int k = 0; k < HC_MAX_VISC_CLASSES; k++) v.omega_class[k] = k < L->visc_n ? L->visc_omega[k] : L->omega;
  return v;
}

dim3 plane_grid(const hc_lattice *L, int nplanes) { return dim3((unsigned)((L->plane + 255) / 256), (unsigned)nplanes, 1); }

int ensure_scratch(hc_lattice *L, size_t doubles) { return L->scratch.reserve(doubles); }

// (re)build the active-span map from the host mask classes
int rebuild_active_map(hc_lattice *L) {
  const int NX = L->nx + 2 * HALO, ny = L->ny, nz = L->nz;
  std::vector<int> z0((size_t)NX * ny), cum((size_t)NX * (ny + 1));
  int max_active = 0;
  for (int x = 0; x < NX; x++) {
    int c = 0;
    for (int y = 0; y < ny; y++) {
      const uint8_t *row = L->hmask.data() + (size_t)x * L->xs + (size_t)y * nz;
      int a = 0, b = nz;
      while (a < nz && row[a] == 2) a++;
      while (b > a && row[b - 1] == 2) b--;
      z0[(size_t)x * ny + y] = a;
      cum[(size_t)x * (ny + 1) + y] = c;
      c += b - a;
    }
    cum[(size_t)x * (ny + 1) + ny] = c;
    max_active = std::max(max_active, c);
  }
  if (max_active == 0) max_active = 1;
  const int nblk = (max_active + 255) / 256;
  std::vector<int> blk((size_t)NX * (nblk + 1));
  for (int x = 0; x < NX; x++) {
    const int *cx = cum.data() + (size_t)x * (ny + 1);
    int y = 0;
    for (int b = 0; b <= nblk; b++) {
      const long t = (long)b * 256;
      while (y + 1 < ny && cx[y + 1] <= t) y++;
      blk[(size_t)x * (nblk + 1) + b] = y;
    }
  }
  for (hc::DevBuf<int> *b : {&L->row_z0, &L->row_cum, &L->blk_row}) b->reset();   // new blocks every time: the free waits for kernels that read the old map
  int rc;
  if ((rc = L->row_z0.reserve(z0.size())) != HC_OK || (rc = L->row_cum.reserve(cum.size())) != HC_OK || (rc = L->blk_row.reserve(blk.size())) != HC_OK) return rc;
  HC_HIP(hipMemcpy(L->row_z0, z0.data(), z0.size() * sizeof(int), hipMemcpyHostToDevice));
  HC_HIP(hipMemcpy(L->row_cum, cum.data(), cum.size() * sizeof(int), hipMemcpyHostToDevice));
  HC_HIP(hipMemcpy(L->blk_row, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
  L->nblk = nblk; L->max_active = max_active;
  return HC_OK;
}

// one byte per 8 x 8 x 8 brick (see hc_lattice::wallbrick)
int rebuild_wall_bricks(hc_lattice *L) {
  const int NX = L->nx + 2 * HALO, ny = L->ny, nz = L->nz;
  std::vector<uint8_t> flag((size_t)L->nbx * L->nby * L->nbz, 0);
  for (int bx = 0; bx < L->nbx; bx++)
    for (int by = 0; by < L->nby; by++)
      for (int bz = 0; bz < L->nbz; bz++) {
        bool near = false;
        // faces no stencil crosses: the ends of a non-periodic axis; the halo planes of a slab (a single slab never addresses them)
        if (!L->periodic[1] && (by == 0 || by == L->nby - 1)) near = true;
        if (!L->periodic[2] && (bz == 0 || bz == L->nbz - 1)) near = true;
        if (bx * 8 < HALO + 1 || bx * 8 + 7 >= L->nx + HALO - 1) near = true;
        for (int x = bx * 8; x < std::min(NX, bx * 8 + 8) && !near; x++)
          for (int y = by * 8; y < std::min(ny, by * 8 + 8) && !near; y++) {
            const uint8_t *row = L->hmask.data() + (size_t)x * L->xs + (size_t)y * nz;
            for (int z = bz * 8; z < std::min(nz, bz * 8 + 8); z++) if (row[z] != 0) { near = true; break; }
          }
        flag[((size_t)bx * L->nby + by) * L->nbz + bz] = near ? 1 : 0;
      }
  { const int rc = L->wallbrick.reserve(flag.size()); if (rc != HC_OK) return rc; }
  HC_HIP(hipMemcpy(L->wallbrick, flag.data(), flag.size(), hipMemcpyHostToDevice));
  return HC_OK;
}

// planes [x_begin, x_begin + nplanes) and, in the same launch, [x2, x2 + n2) (n2 = 0: one range)
int launch_collide(hc_lattice *L, int x_begin, int nplanes, int x2 = 0, int n2 = 0) {
  if (nplanes + n2 <= 0) return HC_OK;
  LatArgs a = make_args(L);
  a.x_begin = x_begin;
  if (n2 > 0) { a.x_split = nplanes; a.x_jump = x2 - (x_begin + nplanes); }
  const unsigned ny = (unsigned)(nplanes + n2);
  const dim3 grid((unsigned)((L->max_active + 255) / 256), ny, 1);
  if (L->visc_n > 0) {   // never together with open-boundary nodes (hcl_interior_enable, ob_add)
    hc::prof_count(hc::PK_COLLIDE_VISC);   // which instantiation ran: a count, no events of its own inside the caller's collide_stream bracket
    const ViscArgs v = visc_of(L, a);
    if (L->regions.n) hipLaunchKernelGGL((collide_stream_kernel<true, false, true>), grid, dim3(256), 0, hc::stream(), v);
    else hipLaunchKernelGGL((collide_stream_kernel<false, false, true>), grid, dim3(256), 0, hc::stream(), v);
    HC_HIP(hipGetLastError());
    return HC_OK;
  }
  launch_open(L, a, [&](auto open, const auto &args) {
    constexpr bool OPEN = decltype(open)::value;
    if (L->regions.n) hipLaunchKernelGGL((collide_stream_kernel<true, OPEN>), grid, dim3(256), 0, hc::stream(), args);
    else hipLaunchKernelGGL((collide_stream_kernel<false, OPEN>), grid, dim3(256), 0, hc::stream(), args);
  });
  HC_HIP(hipGetLastError());
  return HC_OK;
}

int launch_lees_edwards(hc_lattice *L) {
  hc::ProfScope prof(hc::PK_LEES_EDWARDS);
  LatArgs a = make_args(L);
  a.fout = L->f[L->cur];   // the buffer the next collide reads: a.fin
  const long nthreads = 2L * L->nx * L->ny;
  const dim3 grid((unsigned)((nthreads + 255) / 256));
  hipLaunchKernelGGL(le_gather_kernel, grid, dim3(256), 0, hc::stream(), a, L->le_buf, L->le_D, L->le_v_top, L->le_v_bottom);
  HC_HIP(hipGetLastError());
  hipLaunchKernelGGL(le_scatter_kernel, grid, dim3(256), 0, hc::stream(), a, (const double *)L->le_buf);
  HC_HIP(hipGetLastError());
  return HC_OK;
}

}  // namespace

int hc::lees_edwards_step(hc_lattice *L) { return L->le_on ? launch_lees_edwards(L) : HC_OK; }

// the (handle, lattice) pairs of the live pre-inlet handles (common.h).  Not locked: like the error string and the stream
// selection of runtime.hip, the library's entry points are called from one thread.  A counter in hc_lattice would need the
// handles to go before their lattices, and callers release them in either order.
static std::vector<std::pair<const void *, const hc_lattice *>> g_preinlet_pairs;
void hc::preinlet_pair_add(const void *owner, const hc_lattice *L) { g_preinlet_pairs.emplace_back(owner, L); }
void hc::preinlet_pair_remove(const void *owner) {
  g_preinlet_pairs.erase(std::remove_if(g_preinlet_pairs.begin(), g_preinlet_pairs.end(), [&](const auto &e) { return e.first == owner; }), g_preinlet_pairs.end());
}
void hc::preinlet_pair_forget(const hc_lattice *L) {
  g_preinlet_pairs.erase(std::remove_if(g_preinlet_pairs.begin(), g_preinlet_pairs.end(), [&](const auto &e) { return e.second == L; }), g_preinlet_pairs.end());
}
bool hc::in_preinlet_pair(const hc_lattice *L) {
  return std::any_of(g_preinlet_pairs.begin(), g_preinlet_pairs.end(), [&](const auto &e) { return e.second == L; });
}
static std::vector<std::pair<const void *, const hc_lattice *>> g_ibm_wide;
void hc::ibm_wide_add(const void *owner, const hc_lattice *L) { g_ibm_wide.emplace_back(owner, L); }
void hc::ibm_wide_remove_one(const void *owner) {
  const auto it = std::find_if(g_ibm_wide.begin(), g_ibm_wide.end(), [&](const auto &e) { return e.first == owner; });
  if (it != g_ibm_wide.end()) g_ibm_wide.erase(it);
}
void hc::ibm_wide_remove(const void *owner) {
  g_ibm_wide.erase(std::remove_if(g_ibm_wide.begin(), g_ibm_wide.end(), [&](const auto &e) { return e.first == owner; }), g_ibm_wide.end());
}
void hc::ibm_wide_forget(const hc_lattice *L) {
  g_ibm_wide.erase(std::remove_if(g_ibm_wide.begin(), g_ibm_wide.end(), [&](const auto &e) { return e.second == L; }), g_ibm_wide.end());
}
bool hc::ibm_wide(const hc_lattice *L) {
  return std::any_of(g_ibm_wide.begin(), g_ibm_wide.end(), [&](const auto &e) { return e.second == L; });
}

// the four z-layers a Lees-Edwards pass reads or writes populations of (z = 0, 1, nz-2, nz-1): every bulk node there must
// be fluid, so that each stored slot the pass writes has the one reader the pass means (mask: device numbering)
static bool le_layers_fluid(const hc_lattice *L, const uint8_t *mask, size_t xs) {
  const int zs[4] = {0, 1, L->nz - 2, L->nz - 1};
  for (int x = HALO; x < L->nx + HALO; x++)
    for (int y = 0; y < L->ny; y++)
      for (int k = 0; k < 4; k++)
        if (mask[(size_t)x * xs + (size_t)y * L->nz + zs[k]] != 0) return false;
  return true;
}

// The body of the hcl_download_* entry points: per_node doubles for every bulk node are written to the scratch buffer by
// launch(scratch, bulk nodes) and copied from there to the host blocks of dst, one after the other.  refresh_halos: the kernel
// gathers, and on a slab the post-stream view of the face planes pulls from the halo planes.
struct HostBlock { double *ptr; size_t per_node; };
template <class Launch>
static int download(hc_lattice *L, bool refresh_halos, std::initializer_list<HostBlock> dst, Launch launch) {
  if (refresh_halos && L->n_slabs > 1) { const int rc = hcl_slab_refresh_halos(L, 2); if (rc != HC_OK) return rc; }
  const size_t n = (size_t)L->nx * L->plane;
  size_t per_node = 0;
  for (const HostBlock &b : dst) per_node += b.per_node;
  const int rc = ensure_scratch(L, n * per_node); if (rc != HC_OK) return rc;
  launch(L->scratch, n);
  HC_HIP(hipGetLastError());
  const double *src = L->scratch;
  for (const HostBlock &b : dst) {
    HC_HIP(hipMemcpyAsync(b.ptr, src, n * b.per_node * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
    src += n * b.per_node;
  }
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

static int g_force_plane_padding = 0;   // tests / A-B runs: 1 = pad the planes of every lattice, -1 = of none, 0 = by size

extern "C" {

int hc_debug_force_plane_padding(int on) { g_force_plane_padding = on > 0 ? 1 : (on < 0 ? -1 : 0); return HC_OK; }

int hcl_create(hc_lattice **out, int nx, int ny, int nz, const int periodic[3], double omega,
               int x0, int nx_global, int n_slabs) {
  HC_REQUIRE(out && periodic, "hcl_create: null pointer");
  HC_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "hcl_create: every dimension must be >= 2");
  HC_REQUIRE(n_slabs >= 1 && nx_global >= nx && x0 >= 0 && x0 + nx <= nx_global, "hcl_create: inconsistent slab decomposition");
  HC_REQUIRE((long)ny * nz < (1L << 30) && (long)(nx + 2 * HALO) * (((long)ny + 8) * nz + 32) < (1L << 31), "hcl_create: slab too large for 32-bit plane indexing");
  HC_REQUIRE(omega > 0.0 && omega < 2.0, "hcl_create: omega must be in (0,2)");
  if (hc::stream() == nullptr) { hc::set_error("hcl_create: hc_init() has not been called"); return HC_ERR_STATE; }
  std::unique_ptr<hc_lattice> owner(new hc_lattice());   // an early return below frees whatever exists by then
  hc_lattice *L = owner.get();
  L->nx = nx; L->ny = ny; L->nz = nz;
  for (int d = 0; d < 3; d++) L->periodic[d] = periodic[d] ? 1 : 0;
  L->x0 = x0; L->nx_global = nx_global; L->n_slabs = n_slabs;
  L->omega = omega;
  L->plane = (size_t)ny * nz;
  // x-plane stride.  (1) A multiple of 16 doubles, so that the x-1 / x+1 neighbours of a 128-byte line are lines too: with
  // an odd plane (the reference's voxelised tubes are 2N+3 x N+3 x N+3 nodes) every read of a population that moves along
  // x straddles one line more (511 x 257 x 257 pipe: -8 % against 512 x 256 x 257).  (2) x-planes whose size is a multiple
  // of 1 MiB (512 x 512 doubles) put the x-1 / x / x+1 planes a kernel streams at the same time at the same offset in the
  // HBM channel interleave; 8 rows of padding between planes take them apart (all-fluid 512^3 box: about +5 %).
  L->xs = (L->plane + 15) / 16 * 16;
  if (g_force_plane_padding > 0 || (g_force_plane_padding == 0 && ((L->plane * sizeof(double)) % (1u << 20)) == 0)) L->xs += (size_t)(8 * nz + 15) / 16 * 16;
  if (g_force_plane_padding < 0) L->xs = L->plane;
  L->npad = (size_t)(nx + 2 * HALO) * L->xs;
  // The 19 population arrays are streamed side by side.  With power-of-two planes (512 x 512 doubles = 2 MiB) and
  // npad a multiple of the plane, all 38 read / write streams of a node sit at the same offset modulo 2 MiB and
  // camp on the same HBM channels (all-fluid 512^3 box: 5.27 TB/s algorithmic against 6.0 for 256^3).  An odd
  // number of 128-byte lines between consecutive populations spreads them over the channels.
  L->qstride = L->npad + 16 * 129;
  L->cur = 0; L->fcur = 0; L->ibm = 0;
  L->body[0] = L->body[1] = L->body[2] = 0.0;
  L->regions.n = 0;
  for (int c = 0; c < 4; c++) for (int d = 0; d < 3; d++) L->wall_u[c][d] = 0.0;
  int rc;
  for (int k = 0; k < 2; k++) {
    if ((rc = L->f[k].reserve(L->qstride * HC_Q)) != HC_OK) return rc;
    HC_HIP(hipMemsetAsync(L->f[k], 0, L->qstride * HC_Q * sizeof(double), hc::stream()));
  }
  for (int k = 0; k < 3; k++) {
    if ((rc = L->force[k].reserve(L->npad * 3)) != HC_OK) return rc;
    HC_HIP(hipMemsetAsync(L->force[k], 0, L->npad * 3 * sizeof(double), hc::stream()));
  }
  if ((rc = L->mask.reserve(L->npad)) != HC_OK) return rc;
  HC_HIP(hipMemsetAsync(L->mask, 0, L->npad, hc::stream()));
  for (int k = 0; k < 3; k++) {
    if ((rc = L->fdirty[k].reserve(L->npad / 16 + 1)) != HC_OK) return rc;
    HC_HIP(hipMemsetAsync(L->fdirty[k], 0, L->npad / 16 + 1, hc::stream()));
    L->fepoch[k] = 1;
  }
  L->hmask.assign(L->npad, 0);   // device numbering; hcl_set_mask marks the padding
  L->nbx = (nx + 2 * HALO + 7) / 8; L->nby = (ny + 7) / 8; L->nbz = (nz + 7) / 8;
  if ((rc = rebuild_active_map(L)) != HC_OK || (rc = rebuild_wall_bricks(L)) != HC_OK) return rc;
  HC_HIP(hipStreamSynchronize(hc::stream()));
  *out = owner.release();
  return HC_OK;
}

int hcl_destroy(hc_lattice *L) {
  if (!L) return HC_OK;
  HC_REQUIRE(!L->stats, "hcl_destroy: an hc_stats refers to the lattice; destroy it first (hc_stats_destroy)");
  hcs::lattice_destroyed(L);
  hc::scalar_lattice_destroyed(L);
  hc::preinlet_pair_forget(L);
  hc::ibm_wide_forget(L);
  hipStreamSynchronize(hc::stream());
  delete L;
  return HC_OK;
}

int hcl_dims(const hc_lattice *L, int dims[3]) {
  HC_REQUIRE(L && dims, "hcl_dims: null pointer");
  dims[0] = L->nx; dims[1] = L->ny; dims[2] = L->nz;
  return HC_OK;
}

int hcl_node_counts(const hc_lattice *L, long counts[3]) {
  HC_REQUIRE(L && counts, "hcl_node_counts: null pointer");
  long fluid = 0, active = 0;
  for (int x = 0; x < L->nx; x++)
    for (size_t p = 0; p < L->plane; p++) {
      const uint8_t m = L->hmask[(size_t)(x + HALO) * L->xs + p];
      fluid += m == 0; active += m != 2;
    }
  counts[0] = (long)L->nx * (long)L->plane; counts[1] = fluid; counts[2] = active;
  return HC_OK;
}

int hcl_set_mask(hc_lattice *L, const uint8_t *mask_with_halo) {
  HC_REQUIRE(L && mask_with_halo, "hcl_set_mask: null pointer");
  if (L->le_on && !le_layers_fluid(L, mask_with_halo, L->plane)) {
    hc::set_error("hcl_set_mask: the lattice has a Lees-Edwards boundary; the layers z = 0, 1, nz-2 and nz-1 must hold fluid nodes only");
    return HC_ERR_STATE;
  }
  // host copy in the device numbering (x-planes xs apart); the padding between planes is inert solid
  L->hmask.assign(L->npad, 2);
  for (int x = 0; x < L->nx + 2 * HALO; x++)
    for (size_t p = 0; p < L->plane; p++) {
      const uint8_t m = mask_with_halo[(size_t)x * L->plane + p];
      L->hmask[(size_t)x * L->xs + p] = (m >= 3 && m <= 6) ? m : (m ? 1 : 0);   // 1 = bounce-back, 3..6 = moving-wall classes
    }
  // class 2 = solid node without any fluid neighbour.  Full-way bounce-back returns every population to
  // where it came from, so such a node never exchanges anything with the fluid: the collide kernel skips
  // it (no loads, no stores).  Results on fluid nodes are unchanged, bit for bit.
  {
    const int NX = L->nx + 2 * HALO, ny = L->ny, nz = L->nz;
    std::vector<uint8_t> cls(L->hmask);
    for (int x = 0; x < NX; x++)
      for (int y = 0; y < ny; y++)
        for (int z = 0; z < nz; z++) {
          const size_t k = (size_t)x * L->xs + (size_t)y * nz + z;
          if (!L->hmask[k]) continue;
          bool fluid_near = false;
          for (int q = 1; q < HC_Q && !fluid_near; q++) {
            int xx = x + HC_CX[q], yy = y + HC_CY[q], zz = z + HC_CZ[q];
            if (xx < 0 || xx >= NX) { fluid_near = true; break; }   // beyond the halo: unknown, keep the node active
            if (yy < 0 || yy >= ny) { if (L->periodic[1]) yy = (yy + ny) % ny; else continue; }
            if (zz < 0 || zz >= nz) { if (L->periodic[2]) zz = (zz + nz) % nz; else continue; }
            if (!L->hmask[(size_t)xx * L->xs + (size_t)yy * nz + zz]) fluid_near = true;
          }
          if (!fluid_near) cls[k] = 2;
        }
    // a 128-byte line (16 doubles) of a population array must be written completely or not at all:
    // partially written lines at the ends of the live spans cost a read-modify-write in the memory system
    // (measured: the pipe ran no faster than a full box although it moves 18 % fewer bytes).  Inert nodes
    // that share a line with a live node are therefore kept as ordinary bounce-back nodes.
    const size_t n = cls.size();
    for (size_t g = 0; g < n; g += 16) {
      const size_t e = std::min(n, g + 16);
      bool live = false;
      for (size_t k = g; k < e; k++) if (cls[k] != 2) { live = true; break; }
      if (live) for (size_t k = g; k < e; k++) if (cls[k] == 2) cls[k] = 1;
    }
    L->hmask.swap(cls);
  }
  { int rc = rebuild_active_map(L); if (rc != HC_OK) return rc; }
  { int rc = rebuild_wall_bricks(L); if (rc != HC_OK) return rc; }
  HC_HIP(hipMemcpyAsync(L->mask, L->hmask.data(), L->npad, hipMemcpyHostToDevice, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcl_init_equilibrium(hc_lattice *L, double rho, const double u[3]) {
  HC_REQUIRE(L && u, "hcl_init_equilibrium: null pointer");
  LatArgs a = make_args(L);
  a.fout = L->f[L->cur];
  HC_HIP(hipMemsetAsync(L->f[0], 0, L->qstride * HC_Q * sizeof(double), hc::stream()));
  HC_HIP(hipMemsetAsync(L->f[1], 0, L->qstride * HC_Q * sizeof(double), hc::stream()));
  hipLaunchKernelGGL(init_eq_kernel, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), a, rho - 1.0, rho * u[0], rho * u[1], rho * u[2]);
  HC_HIP(hipGetLastError());
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcl_set_wall_velocity(hc_lattice *L, int wall_class, const double u[3]) {
  HC_REQUIRE(L && u && wall_class >= 3 && wall_class <= 6, "hcl_set_wall_velocity: class must be 3..6");
  for (int d = 0; d < 3; d++) L->wall_u[wall_class - 3][d] = u[d];
  return HC_OK;
}

int hcl_set_body_force(hc_lattice *L, const double F[3]) {
  HC_REQUIRE(L && F, "hcl_set_body_force: null pointer");
  for (int d = 0; d < 3; d++) L->body[d] = F[d];
  return HC_OK;
}

int hcl_set_body_force_regions(hc_lattice *L, int n, const int *boxes, const double *forces) {
  HC_REQUIRE(L && n >= 0 && (n == 0 || (boxes && forces)), "hcl_set_body_force_regions: bad arguments");
  HC_REQUIRE(n <= HC_MAX_FORCE_REGIONS, "hcl_set_body_force_regions: more than HC_MAX_FORCE_REGIONS boxes");
  for (int k = 0; k < n; k++) {
    const int *b = boxes + 6 * k;
    HC_REQUIRE(b[0] <= b[1] && b[2] <= b[3] && b[4] <= b[5], "hcl_set_body_force_regions: empty box");
    for (int i = 0; i < 6; i++) L->regions.box[k][i] = b[i];
    for (int d = 0; d < 3; d++) L->regions.f[k][d] = forces[3 * k + d];
  }
  L->regions.n = n;
  return HC_OK;
}

int hcl_collide_stream_part(hc_lattice *L, int part) {
  HC_REQUIRE(L, "hcl_collide_stream_part: null lattice");
  HC_REQUIRE(part >= 0 && part <= 6, "hcl_collide_stream_part: part must be 0..6");
  HC_REQUIRE(part < 3 || L->nx >= 4, "hcl_collide_stream_part: parts 3, 4 and 6 need a slab of at least 4 planes");
  hc::ProfScope prof(hc::forked() ? hc::PK_COLLIDE_BESIDE : hc::PK_COLLIDE);
  int rc = HC_OK;
  if (part == 0) rc = launch_collide(L, 0, L->nx);
  else if (part == 1) rc = launch_collide(L, 1, L->nx - 2);
  else if (part == 2 || part == 5) rc = launch_collide(L, 0, 1, L->nx - 1, 1);       // both face planes in one launch
  else if (part == 3) rc = launch_collide(L, 2, L->nx - 4);
  else rc = launch_collide(L, 0, 2, L->nx - 2, 2);                                  // the two planes next to each face in one launch
  if (rc == HC_OK && (part == 0 || part == 2 || part == 4)) rc = hcl_zero_force_halos(L);
  return rc;
}

// The collide kernel zeroes the other-parity IBM force on the bulk planes; envelope copies of cells also spread onto the halo
// planes, which have to be cleared as well (one small launch; before hcl_step_end of the same step).  Parts 0, 2 and 4 of
// hcl_collide_stream_part do it themselves; after parts 5 / 6 (the slab schedule) the caller does, once its face message is away.
int hcl_zero_force_halos(hc_lattice *L) {
  HC_REQUIRE(L, "hcl_zero_force_halos: null lattice");
  if (L->n_slabs <= 1 || !L->ibm) return HC_OK;
  hipLaunchKernelGGL(zero_force_halo_kernel, dim3((unsigned)((3 * L->plane + 255) / 256), (unsigned)(2 * HALO), 1), dim3(256), 0, hc::stream(),
                     L->force[(L->fcur + 2) % 3], (long)L->xs, (int)L->plane, L->nx);
  HC_HIP(hipGetLastError());
  return HC_OK;
}

int hcl_step_end(hc_lattice *L) {
  HC_REQUIRE(L, "hcl_step_end: null lattice");
  L->cur ^= 1; L->fcur = (L->fcur + 1) % 3;
  L->halo_u_valid = false;   // velocities of a neighbour's face plane belong to the state that has just been replaced
  L->fepoch[L->fcur] = (uint8_t)(L->fepoch[L->fcur] % 255 + 1);   // the buffer spread will add to next gets a fresh epoch (1..255)
  return HC_OK;
}

int hcl_collide_stream(hc_lattice *L, int nsteps) {
  HC_REQUIRE(L, "hcl_collide_stream: null lattice");
  if (L->n_slabs > 1) return hcs::collide_stream_slab(L, nsteps);   // faces exchanged inside, beside the interior collide
  for (int s = 0; s < nsteps; s++) {
    int rc = hcl_collide_stream_part(L, 0);
    if (rc != HC_OK) return rc;
    hcl_step_end(L);
    if ((rc = hc::lees_edwards_step(L)) != HC_OK) return rc;   // Palabos runs the LE processors after the stream; D stays as it is
  }
  return HC_OK;
}

int hcl_set_lees_edwards(hc_lattice *L, double v_top, double v_bottom) {
  HC_REQUIRE(L, "hcl_set_lees_edwards: null lattice");
  HC_REQUIRE(L->n_slabs == 1, "hcl_set_lees_edwards: the Lees-Edwards boundary needs the whole domain on one GPU (n_slabs = 1)");
  HC_REQUIRE(L->periodic[0] && L->periodic[1] && L->periodic[2], "hcl_set_lees_edwards: the lattice must be periodic on all three axes");
  HC_REQUIRE(L->nz >= 4, "hcl_set_lees_edwards: nz must be at least 4");
  HC_REQUIRE(L->ob_n == 0, "hcl_set_lees_edwards: the lattice has open-boundary nodes; open boundaries and Lees-Edwards do not combine");
  HC_REQUIRE(L->visc_n == 0, "hcl_set_lees_edwards: the lattice has interior viscosity enabled; interior viscosity and Lees-Edwards do not combine");
  HC_REQUIRE(!L->scalar, "hcl_set_lees_edwards: the lattice has a scalar field; the scalar field and Lees-Edwards do not combine");
  if (!le_layers_fluid(L, L->hmask.data(), L->xs)) {
    hc::set_error("hcl_set_lees_edwards: the layers z = 0, 1, nz-2 and nz-1 must hold fluid nodes only");
    return HC_ERR_STATE;
  }
  { const int rc = L->le_buf.reserve((size_t)2 * HC_Q * L->nx * L->ny); if (rc != HC_OK) return rc; }
  L->le_on = true; L->le_v_top = v_top; L->le_v_bottom = v_bottom; L->le_D = 0.0; L->le_d = 0.0;
  return HC_OK;
}

int hcl_set_lees_edwards_displacement(hc_lattice *L, double D, double d_per_iteration) {
  HC_REQUIRE(L, "hcl_set_lees_edwards_displacement: null lattice");
  if (!L->le_on) { hc::set_error("hcl_set_lees_edwards_displacement: no Lees-Edwards boundary (hcl_set_lees_edwards)"); return HC_ERR_STATE; }
  L->le_D = D; L->le_d = d_per_iteration;
  return HC_OK;
}

int hcl_lees_edwards_apply(hc_lattice *L) {
  HC_REQUIRE(L, "hcl_lees_edwards_apply: null lattice");
  if (!L->le_on) { hc::set_error("hcl_lees_edwards_apply: no Lees-Edwards boundary (hcl_set_lees_edwards)"); return HC_ERR_STATE; }
  return launch_lees_edwards(L);
}

int hcl_lees_edwards_state(const hc_lattice *L, double out[4]) {
  HC_REQUIRE(L && out, "hcl_lees_edwards_state: null pointer");
  if (!L->le_on) { hc::set_error("hcl_lees_edwards_state: no Lees-Edwards boundary (hcl_set_lees_edwards)"); return HC_ERR_STATE; }
  out[0] = L->le_D; out[1] = L->le_v_top; out[2] = L->le_v_bottom; out[3] = L->le_d;
  return HC_OK;
}

// ---- Zou-He open boundaries (the completion is zou_he_node inside the collide)
// room for `need` slots; the slots from ob_n on start at u = 0, rho = 1
static int ob_grow(hc_lattice *L, int need) {
  if (need <= L->ob_n) return HC_OK;
  const int cap = need <= L->ob_cap ? L->ob_cap : std::max(need, 2 * L->ob_cap);
  hc::DevBuf<double> grown;   // the larger block, while the old one still holds the slots to carry over
  double *v = L->ob_val;
  if (cap > L->ob_cap) {
    const int rc = grown.reserve((size_t)cap * 4); if (rc != HC_OK) return rc;
    v = grown;
    if (L->ob_val && L->ob_n) HC_HIP(hipMemcpyAsync(v, L->ob_val, (size_t)L->ob_n * 4 * sizeof(double), hipMemcpyDeviceToDevice, hc::stream()));
  }
  std::vector<double> init((size_t)(need - L->ob_n) * 4, 0.0);
  for (size_t i = 0; i < init.size(); i += 4) init[i + 3] = 1.0;   // u = 0, rho = 1
  HC_HIP(hipMemcpyAsync(v + (size_t)L->ob_n * 4, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  if (grown) { L->ob_val = std::move(grown); L->ob_cap = cap; }   // the old block is freed on return, after the wait above
  return HC_OK;
}

static int ob_set(hc_lattice *L, const char *what, int first, int n, const double *src, int c0, int nc, int on_device) {
  if (!L || (n > 0 && !src)) { hc::set_error(std::string(what) + ": null pointer"); return HC_ERR_ARG; }
  if (first < 0 || n < 0 || first + n > L->ob_n) { hc::set_error(std::string(what) + ": slots out of range"); return HC_ERR_ARG; }
  if (n == 0) return HC_OK;
  const double *d = src;
  if (!on_device) {
    int rc = ensure_scratch(L, (size_t)n * nc); if (rc != HC_OK) return rc;
    HC_HIP(hipMemcpyAsync(L->scratch, src, (size_t)n * nc * sizeof(double), hipMemcpyHostToDevice, hc::stream()));
    d = L->scratch;
  }
  hipLaunchKernelGGL(ob_set_kernel, dim3((unsigned)((n * nc + 255) / 256)), dim3(256), 0, hc::stream(), L->ob_val, first, n, d, c0, nc);
  HC_HIP(hipGetLastError());
  if (!on_device) HC_HIP(hipStreamSynchronize(hc::stream()));   // the host buffer may go away after the call
  return HC_OK;
}

// is the bulk node c = {x, y, z} inside the lattice?  *index: its element in the device numbering
static bool ob_node(const hc_lattice *L, const int *c, size_t *index) {
  *index = (size_t)(c[0] + HALO) * L->xs + (size_t)c[1] * L->nz + c[2];
  return c[0] >= 0 && c[0] < L->nx && c[1] >= 0 && c[1] < L->ny && c[2] >= 0 && c[2] < L->nz;
}

// who: the entry point the caller used, for the messages
static int ob_add(const std::string &who, hc_lattice *L, int kind, int axis, int orientation, const int *nodes, int n, int *first_slot) {
  HC_REQUIRE(L && (n == 0 || nodes), who + ": null pointer");
  // A slab declares its own nodes, in local coordinates and with slots of its own.  The completion touches the node's gathered
  // populations only, and on a face plane those have crossed with the step's face message (an x-normal node at a domain end
  // gathers the zeros of a halo plane nobody fills, as the single domain does), so nothing else of the schedule changes.
  // Like every step and observer of a slab, the declaration belongs to a connected run: a lone lattice that merely names
  // n_slabs > 1 is refused as it always was.
  HC_REQUIRE(L->n_slabs == 1 || hcm::active(), who + ": open boundaries on a lattice with n_slabs > 1 need the ranks connected first (hc_comm_init_env / hc_comm_init); an unconnected lattice takes them with n_slabs = 1");
  HC_REQUIRE(kind == HC_OB_VELOCITY || kind == HC_OB_PRESSURE, who + ": kind must be HC_OB_VELOCITY or HC_OB_PRESSURE");
  HC_REQUIRE(orientation == -1 || orientation == 1, who + ": orientation must be -1 (N) or +1 (P)");
  HC_REQUIRE(axis >= 0 && axis <= 2, who + ": axis must be 0, 1 or 2");
  HC_REQUIRE(n >= 0 && (long)L->ob_n + n < (long)HC_OB_MAX_SLOTS, who + ": too many nodes");
  // The Lees-Edwards pass rewrites the post-stream populations of its z layers from plain moments of gathered populations; what
  // it should read and leave on a node whose populations the collide completes is not defined, so the two do not share a lattice
  HC_REQUIRE(!L->le_on, who + ": the lattice has a Lees-Edwards boundary; open boundaries and Lees-Edwards do not combine");
  // the open-boundary and the interior-viscosity collide are two instantiations; no kernel does both
  HC_REQUIRE(L->visc_n == 0, who + ": the lattice has interior viscosity enabled; interior viscosity and open boundaries do not combine");
  // the OPEN interpolation exists for the two-point kernels only (hcp_type_set_ibm_kernel)
  HC_REQUIRE(!hc::ibm_wide(L), who + ": a cell type of the lattice is on a three- or four-point IBM kernel; those and open boundaries do not combine");
  // the scalar step takes plain moments of the flow's populations and knows no open faces of its own
  HC_REQUIRE(!L->scalar, who + ": the lattice has a scalar field; the scalar field and open boundaries do not combine");
  // a node holds one slot: declaring it again (in this call or an earlier one) would orphan the first slot and let the second
  // declaration win silently, so it is refused and nothing is changed
  {
    std::vector<size_t> seen((size_t)n);
    for (int i = 0; i < n; i++) {
      HC_REQUIRE(ob_node(L, nodes + 3 * i, &seen[(size_t)i]), who + ": node outside the lattice");
      HC_REQUIRE(!L->ob_code || L->ob_hcode[seen[(size_t)i]] < 0, who + ": node declared twice (it is an open-boundary node already; hcl_open_boundary_clear removes all)");
    }
    std::sort(seen.begin(), seen.end());
    HC_REQUIRE(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), who + ": node declared twice (listed more than once)");
  }
  if (first_slot) *first_slot = L->ob_n;
  if (n == 0) return HC_OK;
  int rc = ob_grow(L, L->ob_n + n); if (rc != HC_OK) return rc;
  if (!L->ob_code) {
    rc = L->ob_code.reserve(L->npad); if (rc != HC_OK) return rc;
    L->ob_hcode.assign(L->npad, -1);
  }
  const int k = (kind == HC_OB_PRESSURE ? 2 : 0) + (orientation > 0 ? 1 : 0);
  for (int i = 0; i < n; i++) {
    size_t node;
    ob_node(L, nodes + 3 * i, &node);   // checked above
    L->ob_hcode[node] = (axis << HC_OB_AXIS_SHIFT) | ((L->ob_n + i) << 2) | k;
  }
  L->ob_n += n;
  HC_HIP(hipMemcpyAsync(L->ob_code, L->ob_hcode.data(), L->npad * sizeof(int), hipMemcpyHostToDevice, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcl_open_boundary_add_axis(hc_lattice *L, int kind, int axis, int orientation, const int *nodes, int n, int *first_slot) {
  return ob_add("hcl_open_boundary_add_axis", L, kind, axis, orientation, nodes, n, first_slot);
}

int hcl_open_boundary_add(hc_lattice *L, int kind, int orientation, const int *nodes, int n, int *first_slot) {
  return ob_add("hcl_open_boundary_add", L, kind, 0, orientation, nodes, n, first_slot);
}

static int ob_add_box(const std::string &who, hc_lattice *L, int kind, int axis, int orientation, const int box[6], int *first_slot, int *n_nodes) {
  HC_REQUIRE(L && box, who + ": null pointer");
  HC_REQUIRE(box[0] <= box[1] && box[2] <= box[3] && box[4] <= box[5], who + ": empty box");
  std::vector<int> nodes;
  for (int x = box[0]; x <= box[1]; x++)
    for (int y = box[2]; y <= box[3]; y++)
      for (int z = box[4]; z <= box[5]; z++) { nodes.push_back(x); nodes.push_back(y); nodes.push_back(z); }
  const int n = (int)(nodes.size() / 3);
  const int rc = ob_add(who, L, kind, axis, orientation, nodes.data(), n, first_slot);
  if (rc == HC_OK && n_nodes) *n_nodes = n;
  return rc;
}

int hcl_open_boundary_add_box_axis(hc_lattice *L, int kind, int axis, int orientation, const int box[6], int *first_slot, int *n_nodes) {
  return ob_add_box("hcl_open_boundary_add_box_axis", L, kind, axis, orientation, box, first_slot, n_nodes);
}

int hcl_open_boundary_add_box(hc_lattice *L, int kind, int orientation, const int box[6], int *first_slot, int *n_nodes) {
  return ob_add_box("hcl_open_boundary_add_box", L, kind, 0, orientation, box, first_slot, n_nodes);
}

int hcl_open_boundary_clear(hc_lattice *L) {
  HC_REQUIRE(L, "hcl_open_boundary_clear: null lattice");
  if (L->ob_code) {
    std::fill(L->ob_hcode.begin(), L->ob_hcode.end(), -1);
    HC_HIP(hipMemcpyAsync(L->ob_code, L->ob_hcode.data(), L->npad * sizeof(int), hipMemcpyHostToDevice, hc::stream()));
    HC_HIP(hipStreamSynchronize(hc::stream()));
  }
  L->ob_n = 0; L->ob_epoch++;
  return HC_OK;
}

// out[i] = part(code of node i), or -1 where the node is outside the lattice or no open-boundary node
static void ob_lookup(const hc_lattice *L, const int *nodes, int n, int (*part)(int), int *out) {
  for (int i = 0; i < n; i++) {
    size_t node;
    const int code = L->ob_code && ob_node(L, nodes + 3 * i, &node) ? L->ob_hcode[node] : -1;
    out[i] = code < 0 ? -1 : part(code);
  }
}

int hcl_open_boundary_slots(const hc_lattice *L, const int *nodes, int n, int *slots) {
  HC_REQUIRE(L && n >= 0 && (n == 0 || (nodes && slots)), "hcl_open_boundary_slots: bad arguments");
  ob_lookup(L, nodes, n, ob_slot, slots);
  return HC_OK;
}

int hcl_open_boundary_axes(const hc_lattice *L, const int *nodes, int n, int *axes) {
  HC_REQUIRE(L && n >= 0 && (n == 0 || (nodes && axes)), "hcl_open_boundary_axes: bad arguments");
  ob_lookup(L, nodes, n, ob_axis, axes);
  return HC_OK;
}

int hcl_open_boundary_set_velocity(hc_lattice *L, int first_slot, int n, const double *u, int on_device) {
  return ob_set(L, "hcl_open_boundary_set_velocity", first_slot, n, u, 0, 3, on_device);
}

int hcl_open_boundary_set_density(hc_lattice *L, int first_slot, int n, const double *rho, int on_device) {
  return ob_set(L, "hcl_open_boundary_set_density", first_slot, n, rho, 3, 1, on_device);
}

int hcl_open_boundary_values(hc_lattice *L, int first_slot, int n, double *out) {
  HC_REQUIRE(L && (n == 0 || out), "hcl_open_boundary_values: null pointer");
  HC_REQUIRE(first_slot >= 0 && n >= 0 && first_slot + n <= L->ob_n, "hcl_open_boundary_values: slots out of range");
  if (n == 0) return HC_OK;
  HC_HIP(hipMemcpyAsync(out, L->ob_val + 4L * first_slot, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

// nodes of the plane coordinate[axis] == const, and the lattice's extent along the axis
static size_t plane_nodes(const hc_lattice *L, int axis) { return axis == 0 ? L->plane : (size_t)L->nx * (axis == 1 ? L->nz : L->ny); }
static int axis_extent(const hc_lattice *L, int axis) { return axis == 0 ? L->nx : axis == 1 ? L->ny : L->nz; }

// plane_velocity_kernel on the plane coordinate[axis] == plane of L: the one place that picks its instantiation
static int launch_plane_velocity(const hc_lattice *L, int axis, int plane, const int *idx, int n, double *out, int stride) {
  const dim3 grid((unsigned)((n + 255) / 256));
  launch_open(L, make_args(L), [&](auto open, const auto &a) {
    constexpr bool OPEN = decltype(open)::value;
    switch (axis) {
      case 0: hipLaunchKernelGGL((plane_velocity_kernel<OPEN, 0>), grid, dim3(256), 0, hc::stream(), a, plane, idx, n, out, stride); break;
      case 1: hipLaunchKernelGGL((plane_velocity_kernel<OPEN, 1>), grid, dim3(256), 0, hc::stream(), a, plane, idx, n, out, stride); break;
      default: hipLaunchKernelGGL((plane_velocity_kernel<OPEN, 2>), grid, dim3(256), 0, hc::stream(), a, plane, idx, n, out, stride); break;
    }
  });
  HC_HIP(hipGetLastError());
  return HC_OK;
}

// who: the entry point the caller used, for the messages
static int plane_velocity(const std::string &who, hc_lattice *L, int axis, int plane, const int *idx, int n, double *out, int on_device) {
  HC_REQUIRE(L && n >= 0 && (n == 0 || (idx && out)), who + ": bad arguments");
  HC_REQUIRE(axis >= 0 && axis <= 2, who + ": axis must be 0, 1 or 2");
  HC_REQUIRE(plane >= 0 && plane < axis_extent(L, axis), who + ": plane outside the lattice");
  HC_REQUIRE(L->n_slabs == 1, who + ": needs n_slabs = 1");
  for (int i = 0; i < n; i++) HC_REQUIRE(idx[i] >= 0 && (size_t)idx[i] < plane_nodes(L, axis), who + ": in-plane index out of range");
  if (n == 0) return HC_OK;
  int rc = L->ob_list.reserve((size_t)n); if (rc != HC_OK) return rc;
  HC_HIP(hipMemcpyAsync(L->ob_list, idx, (size_t)n * sizeof(int), hipMemcpyHostToDevice, hc::stream()));
  double *d = out;
  if (!on_device) { rc = L->ob_out.reserve((size_t)3 * n); if (rc != HC_OK) return rc; d = L->ob_out; }
  if ((rc = launch_plane_velocity(L, axis, plane, L->ob_list, n, d, 3)) != HC_OK) return rc;
  if (!on_device) HC_HIP(hipMemcpyAsync(out, d, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));   // the staged node list is reused by the next call
  return HC_OK;
}

int hcl_plane_velocity(hc_lattice *L, int x, const int *yz, int n, double *out, int on_device) {
  return plane_velocity("hcl_plane_velocity", L, 0, x, yz, n, out, on_device);
}

int hcl_plane_velocity_axis(hc_lattice *L, int axis, int plane, const int *idx, int n, double *out, int on_device) {
  return plane_velocity("hcl_plane_velocity_axis", L, axis, plane, idx, n, out, on_device);
}

// ---- the pre-inlet's fluid coupling on the device (hcl_preinlet_*)
struct hc_preinlet {
  hc_lattice *pre, *domain;   // not owned: the handle is destroyed before either lattice
  int axis, plane;            // the pre-inlet's plane coordinate[axis] == plane ...
  hc::DevBuf<int> idx;        // ... and the in-plane indices of its coupled nodes [n], device
  int n, first;               // the domain's velocity slots first .. first + n - 1
  long epoch;                 // the domain's ob_epoch at creation: hcl_open_boundary_clear moves it on
};

static bool preinlet_slots_gone(const hc_preinlet *P) { return P->epoch != P->domain->ob_epoch || (long)P->first + P->n > (long)P->domain->ob_n; }

// Everything that can change between two calls is taken here, at launch time: the domain's ob_val is reallocated when its
// slots grow, and hcl_open_boundary_clear drops the slots (then nothing is launched, whatever was declared since: the slots
// of a later declaration are not the ones this handle was checked against)
static int preinlet_launch(const char *who, hc_preinlet *P) {
  hc_lattice *pre = P->pre, *dom = P->domain;
  if (preinlet_slots_gone(P)) {
    hc::set_error(std::string(who) + ": the domain no longer holds the coupled slots (open boundaries cleared since hcl_preinlet_create)");
    return HC_ERR_STATE;
  }
  if (P->n == 0) return HC_OK;
  return launch_plane_velocity(pre, P->axis, P->plane, P->idx, P->n, dom->ob_val + 4L * P->first, 4);
}

int hcl_preinlet_create(hc_preinlet **out, hc_lattice *pre, hc_lattice *domain, int axis, int pre_plane,
                        const int *pre_idx, int n, int domain_first_slot) {
  HC_REQUIRE(out && pre && domain && n >= 0 && (n == 0 || pre_idx), "hcl_preinlet_create: bad arguments");
  HC_REQUIRE(axis >= 0 && axis <= 2, "hcl_preinlet_create: axis must be 0, 1 or 2");
  HC_REQUIRE(pre->n_slabs == 1, "hcl_preinlet_create: needs n_slabs = 1 on the pre-inlet lattice");
  HC_REQUIRE(pre->visc_n == 0 && domain->visc_n == 0, "hcl_preinlet_create: a lattice has interior viscosity enabled; interior viscosity and a pre-inlet do not combine");
  HC_REQUIRE(!pre->scalar && !domain->scalar, "hcl_preinlet_create: a lattice has a scalar field; the scalar field and a pre-inlet do not combine");
  HC_REQUIRE(!hc::ibm_wide(pre) && !hc::ibm_wide(domain), "hcl_preinlet_create: a cell type of a lattice is on a three- or four-point IBM kernel; those and a pre-inlet do not combine");
  // a slab domain: the inlet plane of an x direction lies on one rank, whose local slots these are; a y or z plane would span the ranks
  HC_REQUIRE(domain->n_slabs == 1 || axis == 0, "hcl_preinlet_create: axis 1 and 2 need n_slabs = 1 on the domain; a slab domain is coupled along x only (axis 0)");
  HC_REQUIRE(pre_plane >= 0 && pre_plane < axis_extent(pre, axis), "hcl_preinlet_create: plane outside the pre-inlet lattice");
  for (int i = 0; i < n; i++) HC_REQUIRE(pre_idx[i] >= 0 && (size_t)pre_idx[i] < plane_nodes(pre, axis), "hcl_preinlet_create: in-plane index out of range");
  HC_REQUIRE(domain_first_slot >= 0 && (long)domain_first_slot + n <= (long)domain->ob_n, "hcl_preinlet_create: slots out of range on the domain");
  if (n > 0) {   // every coupled slot belongs to a velocity node (kind bit 1 of the code is clear)
    long found = 0;
    for (const int code : domain->ob_hcode) {
      if (code < 0) continue;
      if (ob_slot(code) < domain_first_slot || ob_slot(code) >= domain_first_slot + n) continue;
      HC_REQUIRE(!ob_is_pressure(code), "hcl_preinlet_create: a coupled slot is a pressure slot; the coupling sets velocities");
      found++;
    }
    HC_REQUIRE(found == n, "hcl_preinlet_create: a coupled slot has no node");
  }
  std::unique_ptr<hc_preinlet> P(new hc_preinlet());
  P->pre = pre; P->domain = domain; P->axis = axis; P->plane = pre_plane; P->n = n; P->first = domain_first_slot;
  P->epoch = domain->ob_epoch;
  if (n > 0) {
    const int rc = P->idx.reserve((size_t)n); if (rc != HC_OK) return rc;
    HC_HIP(hipMemcpyAsync(P->idx, pre_idx, (size_t)n * sizeof(int), hipMemcpyHostToDevice, hc::stream()));
    HC_HIP(hipStreamSynchronize(hc::stream()));   // the caller's list may go away after the call
  }
  hc::preinlet_pair_add(P.get(), pre); hc::preinlet_pair_add(P.get(), domain);
  *out = P.release();
  return HC_OK;
}

int hcl_preinlet_apply(hc_preinlet *P) {
  HC_REQUIRE(P, "hcl_preinlet_apply: null handle");
  return preinlet_launch("hcl_preinlet_apply", P);
}

int hcl_preinlet_iterate(hc_preinlet *P, int n) {
  HC_REQUIRE(P && n >= 0, "hcl_preinlet_iterate: bad arguments");
  if (preinlet_slots_gone(P)) return preinlet_launch("hcl_preinlet_iterate", P);   // refused before any step
  for (int it = 0; it < n; it++) {
    int rc = hcl_collide_stream(P->pre, 1); if (rc != HC_OK) return rc;
    if ((rc = hcl_collide_stream(P->domain, 1)) != HC_OK) return rc;
    if ((rc = preinlet_launch("hcl_preinlet_iterate", P)) != HC_OK) return rc;
  }
  return HC_OK;
}

int hcl_preinlet_destroy(hc_preinlet *P) {
  if (!P) return HC_OK;
  hipStreamSynchronize(hc::stream());
  hc::preinlet_pair_remove(P);
  delete P;
  return HC_OK;
}

// ---- interior viscosity: the per-node class field of the collide's VISC instantiation
int hcl_interior_enable(hc_lattice *L, int n_classes, const double *omega) {
  HC_REQUIRE(L && omega, "hcl_interior_enable: null pointer");
  HC_REQUIRE(n_classes >= 1 && n_classes <= HC_MAX_VISC_CLASSES, "hcl_interior_enable: the number of classes must be 1 .. HC_MAX_VISC_CLASSES");
  for (int k = 0; k < n_classes; k++) HC_REQUIRE(omega[k] > 0.0 && omega[k] < 2.0, "hcl_interior_enable: every omega must be in (0,2)");
  HC_REQUIRE(L->n_slabs == 1, "hcl_interior_enable: interior viscosity needs the whole domain on one GPU (n_slabs = 1)");
  HC_REQUIRE(L->ob_n == 0, "hcl_interior_enable: the lattice has open-boundary nodes; interior viscosity and open boundaries do not combine");
  HC_REQUIRE(!L->le_on, "hcl_interior_enable: the lattice has a Lees-Edwards boundary; interior viscosity and Lees-Edwards do not combine");
  HC_REQUIRE(!L->scalar, "hcl_interior_enable: the lattice has a scalar field; the scalar field and interior viscosity do not combine");
  if (!L->visc_class) {   // a second call changes the omegas and keeps the field
    const int rc = L->visc_class.reserve(L->npad); if (rc != HC_OK) return rc;
    HC_HIP(hipMemsetAsync(L->visc_class, 0, L->npad, hc::stream()));
    HC_HIP(hipStreamSynchronize(hc::stream()));
  }
  for (int k = 0; k < n_classes; k++) L->visc_omega[k] = omega[k];
  L->visc_n = n_classes;
  return HC_OK;
}

int hcl_interior_info(const hc_lattice *L, int *n_classes, double *omega) {
  HC_REQUIRE(L && n_classes, "hcl_interior_info: null pointer");
  *n_classes = L->visc_n;
  if (omega) for (int k = 0; k < L->visc_n; k++) omega[k] = L->visc_omega[k];
  return HC_OK;
}

int hcl_interior_upload_classes(hc_lattice *L, const uint8_t *classes) {
  HC_REQUIRE(L && classes, "hcl_interior_upload_classes: null pointer");
  if (L->visc_n == 0) { hc::set_error("hcl_interior_upload_classes: interior viscosity is not enabled (hcl_interior_enable)"); return HC_ERR_STATE; }
  std::vector<uint8_t> h(L->npad, 0);   // device numbering; halo planes and padding stay class 0
  for (int x = 0; x < L->nx; x++)
    for (size_t p = 0; p < L->plane; p++) {
      const uint8_t c = classes[(size_t)x * L->plane + p];
      HC_REQUIRE(c <= L->visc_n, "hcl_interior_upload_classes: a class exceeds the number of enabled classes");
      h[(size_t)(x + HALO) * L->xs + p] = c;
    }
  HC_HIP(hipMemcpyAsync(L->visc_class, h.data(), L->npad, hipMemcpyHostToDevice, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcl_interior_download_classes(hc_lattice *L, uint8_t *classes) {
  HC_REQUIRE(L && classes, "hcl_interior_download_classes: null pointer");
  if (L->visc_n == 0) { hc::set_error("hcl_interior_download_classes: interior viscosity is not enabled (hcl_interior_enable)"); return HC_ERR_STATE; }
  std::vector<uint8_t> h(L->npad);
  HC_HIP(hipMemcpyAsync(h.data(), L->visc_class, L->npad, hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  for (int x = 0; x < L->nx; x++) std::memcpy(classes + (size_t)x * L->plane, h.data() + (size_t)(x + HALO) * L->xs, L->plane);
  return HC_OK;
}

int hcl_download_populations(hc_lattice *L, double *f_aos) {
  HC_REQUIRE(L && f_aos, "hcl_download_populations: null pointer");
  return download(L, true, {{f_aos, HC_Q}}, [&](double *out, size_t) {
    hipLaunchKernelGGL(download_kernel, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), make_args(L), out);
  });
}

int hcl_upload_populations(hc_lattice *L, const double *f_aos) {
  HC_REQUIRE(L && f_aos, "hcl_upload_populations: null pointer");
  const size_t np = (size_t)L->plane * HC_Q, nd = (size_t)L->nx * np;
  int rc = ensure_scratch(L, nd + 2 * np); if (rc != HC_OK) return rc;
  double *bulk = L->scratch + np;   // scratch: plane -1, the nx planes of the slab, plane nx
  HC_HIP(hipMemcpyAsync(bulk, f_aos, nd * sizeof(double), hipMemcpyHostToDevice, hc::stream()));
  int lo_ok = 0, hi_ok = 0;
  if (L->n_slabs > 1) {
    // The stored value of a face node in a direction that crosses the face is the post-stream value of the NEIGHBOUR's first
    // plane: every rank hands its face planes to its neighbours (collective: all ranks of the run upload together, as
    // HemoCell::loadCheckPoint does)
    HC_REQUIRE(hcm::active(), "hcl_upload_populations: a slab of a multi-rank run needs the ranks connected (hc_comm_init) -- the call is collective");
    int lo, hi; hcm::neighbours(L->periodic[0] != 0, lo, hi);
    lo_ok = lo >= 0; hi_ok = hi >= 0;
    rc = hcm::exchange(hc::stream(), L->periodic[0] != 0, bulk, np * sizeof(double), bulk + (size_t)(L->nx - 1) * np, np * sizeof(double), L->scratch, np * sizeof(double),
                       bulk + nd, np * sizeof(double));
    if (rc != HC_OK) return rc;
    hcs::halos_stale(L);
  }
  LatArgs a = make_args(L);
  a.fout = L->f[L->cur];
  hipLaunchKernelGGL(upload_kernel, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), a, (const double *)bulk, lo_ok, hi_ok);
  HC_HIP(hipGetLastError());
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcl_download_rho_u(hc_lattice *L, double *rho, double *u) {
  HC_REQUIRE(L && rho && u, "hcl_download_rho_u: null pointer");
  return download(L, true, {{rho, 1}, {u, 3}}, [&](double *out, size_t n) {
    launch_open(L, make_args(L), [&](auto open, const auto &a) {
      hipLaunchKernelGGL(rho_u_kernel<decltype(open)::value>, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), a, out, out + n);
    });
  });
}

int hcl_download_pi_neq(hc_lattice *L, double *pi) {
  HC_REQUIRE(L && pi, "hcl_download_pi_neq: null pointer");
  return download(L, true, {{pi, 6}}, [&](double *out, size_t) {
    launch_open(L, make_args(L), [&](auto open, const auto &a) {
      hipLaunchKernelGGL(pi_neq_kernel<decltype(open)::value>, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), a, out);
    });
  });
}

int hcl_download_ibm_force(hc_lattice *L, double *F) {
  HC_REQUIRE(L && F, "hcl_download_ibm_force: null pointer");
  return download(L, false, {{F, 3}}, [&](double *out, size_t) {
    hipLaunchKernelGGL(force_aos_kernel, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), make_args(L), out);
  });
}

int hcl_zero_ibm_force(hc_lattice *L) {
  HC_REQUIRE(L, "hcl_zero_ibm_force: null lattice");
  HC_HIP(hipMemsetAsync(L->force[L->fcur], 0, L->npad * 3 * sizeof(double), hc::stream()));
  return HC_OK;
}

int hcl_fluid_stats(hc_lattice *L, int what, double out[3], long *n_nodes) {
  HC_REQUIRE(L && out && n_nodes && what >= 0 && what <= 2, "hcl_fluid_stats: bad arguments");
  if (L->n_slabs > 1 && what == 0) { const int rc0 = hcl_slab_refresh_halos(L, 1); if (rc0 != HC_OK) return rc0; }   // velocities on the face planes pull from the halos
  int rc = ensure_scratch(L, (size_t)STAT_BLOCKS * 4); if (rc != HC_OK) return rc;
  launch_open(L, make_args(L), [&](auto open, const auto &a) {
    hipLaunchKernelGGL(fluid_stats_kernel<decltype(open)::value>, dim3(STAT_BLOCKS), dim3(256), 0, hc::stream(), a, what, L->scratch);
  });
  HC_HIP(hipGetLastError());
  return hc::stat_finish(L->scratch, out, n_nodes);
}

size_t hcl_halo_doubles(const hc_lattice *L, int width) {
  if (!L) return 0;
  return (size_t)(width == 1 ? 5 : 14 + 5) * L->plane;
}

// width 1 (every step): the 5 populations that cross the face.  width 2 (before interpolation): everything the
// neighbour needs to evaluate node velocities on its first halo plane.  S(x, i) = P(x - c_i, i) there pulls the 9 populations
// with c_x = 0 from the face plane itself, the 5 moving towards the neighbour from the plane behind it, and the 5 moving
// away from the neighbour out of the neighbour's own first plane; the neighbour's next collide pulls the 5 moving towards
// it from the face plane.  So 14 populations of the face plane and 5 of the plane behind travel: 19 planes, not 24.
// appends the (population, plane) entries of one face's message to h
static void halo_entries(const hc_lattice *L, int side, int width, int to_buf, HaloArgs &h) {
  static const int cxm[5] = {1, 4, 5, 6, 7};        // c_x = -1
  static const int cxp[5] = {10, 13, 14, 15, 16};   // c_x = +1
  // the populations that travel towards -x (cxm) leave through the low face and arrive in the low neighbour's high
  // halo; those towards +x (cxp) the other way round
  const int *moving = to_buf ? (side == 0 ? cxm : cxp) : (side == 0 ? cxp : cxm);
  // plane next to the face (bulk side when packing, halo side when unpacking) and the one behind it
  const int near = to_buf ? (side == 0 ? HALO : HALO + L->nx - 1) : (side == 0 ? HALO - 1 : HALO + L->nx);
  const int far = to_buf ? (side == 0 ? HALO + 1 : HALO + L->nx - 2) : (side == 0 ? HALO - 2 : HALO + L->nx + 1);
  if (width == 2) {
    for (int q = 0; q < HC_Q; q++)
      if (HC_CX[q] == 0 || HC_CX[q] == HC_CX[moving[0]]) { h.pop[h.n] = q; h.xp[h.n] = near; h.n++; }
  }
  for (int k = 0; k < 5; k++) { h.pop[h.n] = moving[k]; h.xp[h.n] = width == 1 ? near : far; h.n++; }
}
// packs (to_buf) or unpacks the entries of h, entries e >= n_first through buf_hi
static int halo_launch(hc_lattice *L, HaloArgs &h, double *buf, double *buf_hi, int n_first, int to_buf, int next) {
  h.f = L->f[next ? 1 - L->cur : L->cur]; h.buf = buf; h.buf2 = buf_hi; h.n_first = n_first;
  h.npad = (long)L->qstride; h.xs = (long)L->xs; h.plane = (int)L->plane; h.to_buf = to_buf;
  if (h.n == 0) return HC_OK;
  hipLaunchKernelGGL(halo_copy_kernel, dim3((unsigned)((L->plane + 255) / 256), (unsigned)h.n, 1), dim3(256), 0, hc::stream(), h);
  HC_HIP(hipGetLastError());
  return HC_OK;
}
static int halo_copy(hc_lattice *L, int side, int width, double *buf, int to_buf, int next = 0) {
  HC_REQUIRE(L && buf, "hcl_halo: null pointer");
  HC_REQUIRE((side == 0 || side == 1) && (width == 1 || width == 2), "hcl_halo: side must be 0/1 and width 1/2");
  HC_REQUIRE(L->nx >= 2 * width, "hcl_halo: slab thinner than the halo");
  HaloArgs h; h.n = 0;
  halo_entries(L, side, width, to_buf, h);
  return halo_launch(L, h, buf, nullptr, 0x7fffffff, to_buf, next);
}
// the width-1 message of both faces in one launch (either buffer may be null: a slab at a non-periodic end of the domain)
static int halo_copy_both(hc_lattice *L, double *buf_lo, double *buf_hi, int to_buf, int next) {
  HC_REQUIRE(L, "hcl_halo: null pointer");
  HC_REQUIRE(L->nx >= 2, "hcl_halo: slab thinner than the halo");
  HaloArgs h; h.n = 0;
  if (buf_lo) halo_entries(L, 0, 1, to_buf, h);
  if (buf_hi) halo_entries(L, 1, 1, to_buf, h);
  return halo_launch(L, h, buf_lo, buf_hi, buf_lo ? 5 : 0, to_buf, next);
}
int hcl_halo_pack_both(hc_lattice *L, double *dev_lo, double *dev_hi, int next) { return halo_copy_both(L, dev_lo, dev_hi, 1, next); }
int hcl_halo_unpack_both(hc_lattice *L, const double *dev_lo, const double *dev_hi) { return halo_copy_both(L, (double *)dev_lo, (double *)dev_hi, 0, 0); }
int hcl_halo_pack(hc_lattice *L, int side, int width, double *dev_buf) { return halo_copy(L, side, width, dev_buf, 1); }
int hcl_halo_pack_next(hc_lattice *L, int side, int width, double *dev_buf) { return halo_copy(L, side, width, dev_buf, 1, 1); }
int hcl_halo_unpack(hc_lattice *L, int side, int width, const double *dev_buf) { return halo_copy(L, side, width, (double *)dev_buf, 0); }

double hcl_mlups_bytes_per_node(const hc_lattice *L) {
  // 19 reads + 19 writes of fp64 populations and 1 mask byte; with membrane cells bound to the lattice also
  // 3 reads of the IBM force and 3 zeroing writes (304 B fluid only, 353 B coupled)
  return 19 * 8 * 2 + 1 + ((L && L->ibm) ? 3 * 8 * 2 : 0) + ((L && L->visc_n) ? 1 : 0);   // and the class byte with interior viscosity
}

}  // extern "C"

// stats.hip: one sample of the selected fluid sets, queued on the stream in use.  The arguments are those of the observers at
// this moment (make_args): the populations the next collide gathers and the force buffer it reads.
int hc::stats_fluid_sample(hc_lattice *L, int what, double *acc_rho_u, double *acc_uu, double *acc_pi, long stride) {
  launch_open(L, make_args(L), [&](auto open, const auto &a) {
    hipLaunchKernelGGL(stats_fluid_kernel<decltype(open)::value>, plane_grid(L, L->nx), dim3(256), 0, hc::stream(), a, what, acc_rho_u, acc_uu, acc_pi, stride);
  });
  HC_HIP(hipGetLastError());
  return HC_OK;
}
