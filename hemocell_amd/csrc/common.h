// Internal declarations shared by the HIP translation units of libhemocell_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>
#include <type_traits>
#include "../../include/hemocell_amd.h"
#include "d3q19.h"

namespace hc {

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);
hipStream_t stream();
hipStream_t comm_stream();   // third stream: the transfers of slab runs
// fork-join onto the library's side stream: fork() makes the side stream wait for everything enqueued so far,
// route(1) sends the following launches there, route(0) back, join() makes the main stream wait for them
int fork();
void route(int side);
int join();
bool forked();   // between fork() and join()

#define HC_HIP(call)                                                         \
  do {                                                                       \
    hipError_t e__ = (call);                                                 \
    if (e__ != hipSuccess) return hc::hip_fail(e__, #call, __FILE__, __LINE__); \
  } while (0)

#define HC_REQUIRE(cond, msg)                 \
  do {                                        \
    if (!(cond)) {                            \
      hc::set_error(std::string(msg));        \
      return HC_ERR_ARG;                      \
    }                                         \
  } while (0)

// Owning device buffer, pinned host buffer and event.  Move-only; each frees in its destructor and converts to the raw pointer
// or handle, so launch sites and pointer arithmetic read as they do with raw pointers.  reserve(n) returns at once when the
// capacity suffices; otherwise it frees and allocates exactly n elements.  It keeps no old contents, zeroes nothing and waits
// for nothing: the caller chooses the slack, does the wait that must precede the free and any memset.  After a failure the
// buffer is empty.
template <class T> struct DevBuf {
  T *p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept { swap(o); }
  DevBuf &operator=(DevBuf &&o) noexcept { swap(o); return *this; }   // the old block goes with o
  ~DevBuf() { reset(); }
  void swap(DevBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  operator T *() const { return p; }
  int reserve(size_t n) {
    if (n <= cap) return HC_OK;
    reset();
    const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return hip_fail(e, "hipMalloc", __FILE__, __LINE__); }
    cap = n;
    return HC_OK;
  }
};
template <class T> struct PinBuf {
  T *p = nullptr, *dev = nullptr; size_t cap = 0; unsigned flags;   // dev: the device view of a hipHostMallocMapped block
  explicit PinBuf(unsigned f = hipHostMallocDefault) : flags(f) {}
  PinBuf(PinBuf &&o) noexcept : flags(o.flags) { swap(o); }
  PinBuf &operator=(PinBuf &&o) noexcept { swap(o); return *this; }
  ~PinBuf() { reset(); }
  void swap(PinBuf &o) { std::swap(p, o.p); std::swap(dev, o.dev); std::swap(cap, o.cap); std::swap(flags, o.flags); }
  void reset() { if (p) (void)hipHostFree(p); p = dev = nullptr; cap = 0; }
  operator T *() const { return p; }
  int reserve(size_t n) {
    if (n <= cap) return HC_OK;
    reset();
    hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), flags);
    if (e != hipSuccess) p = nullptr;
    else if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer((void **)&dev, p, 0);
    if (e != hipSuccess) { reset(); return hip_fail(e, "hipHostMalloc", __FILE__, __LINE__); }
    cap = n;
    return HC_OK;
  }
};
template <class T> struct MappedBuf : PinBuf<T> { MappedBuf() : PinBuf<T>(hipHostMallocMapped) {} };   // arrays of them need a default constructor
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event &&o) noexcept { std::swap(e, o.e); }
  Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
  int create() {   // on first use; hipEventDisableTiming
    if (e) return HC_OK;
    const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (r != hipSuccess) { e = nullptr; return hip_fail(r, "hipEventCreateWithFlags", __FILE__, __LINE__); }
    return HC_OK;
  }
};
// device block, pinned host block of the same size and the event that guards the pinned block while a copy is in flight
template <class T> struct Staged {
  DevBuf<T> d; PinBuf<T> h; Event ev;
  size_t cap() const { return d.cap < h.cap ? d.cap : h.cap; }
  int reserve(size_t n) { const int rc = d.reserve(n); return rc != HC_OK ? rc : h.reserve(n); }
};

// per-kernel hipEvent timing (hc_profile_*)
enum ProfKernel { PK_COLLIDE = 0, PK_SPREAD, PK_INTERP, PK_ADVANCE, PK_MECH, PK_COLLIDE_BESIDE, PK_LEES_EDWARDS, PK_COLLIDE_VISC, PK_INTERIOR_FIND, PK_INTERIOR_MEMBRANE, PK_SCALAR, PK_SOLIDIFY_PREPARE, PK_SOLIDIFY_FLAG, PK_STATS_FLUID, PK_STATS_DENSITY, PK_STATS_INSIDE, PK_COUNT };   // _BESIDE: collide launches with side-stream work next to them; _VISC: those of the interior-viscosity instantiation, counted a second time (prof_count: no events)
void prof_count(int kernel);   // one more launch of `kernel`, without a time (while profiling is on)
struct ProfScope {
  int k; bool on;
  hipEvent_t a, b;
  explicit ProfScope(int kernel);
  ~ProfScope();
};

constexpr int HALO = 2;  // x-halo planes on each side of a slab

// Deterministic min / max / sum / count reduction used by the statistics entry points: a fixed grid of STAT_BLOCKS
// workgroups, each thread strides over the items, waves combine by shuffles, workgroups write one partial each and
// the host folds the partials in index order.
constexpr int STAT_BLOCKS = 512;
struct StatAcc { double mn, mx, sum; long n; };
__device__ __forceinline__ void stat_add(StatAcc &a, double v) { a.mn = v < a.mn ? v : a.mn; a.mx = v > a.mx ? v : a.mx; a.sum += v; a.n++; }
__device__ __forceinline__ void stat_block_store(StatAcc a, double *partial /*[STAT_BLOCKS][4]*/) {
  __shared__ double s_red[4][4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double mn = __shfl_xor(a.mn, off), mx = __shfl_xor(a.mx, off), sm = __shfl_xor(a.sum, off);
    const long n = __shfl_xor(a.n, off);
    a.mn = mn < a.mn ? mn : a.mn; a.mx = mx > a.mx ? mx : a.mx; a.sum += sm; a.n += n;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_red[w][0] = a.mn; s_red[w][1] = a.mx; s_red[w][2] = a.sum; s_red[w][3] = (double)a.n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double mn = s_red[0][0], mx = s_red[0][1], sm = s_red[0][2], n = s_red[0][3];
    for (int k = 1; k < (int)(blockDim.x >> 6); k++) { mn = s_red[k][0] < mn ? s_red[k][0] : mn; mx = s_red[k][1] > mx ? s_red[k][1] : mx; sm += s_red[k][2]; n += s_red[k][3]; }
    double *o = partial + 4 * blockIdx.x;
    o[0] = mn; o[1] = mx; o[2] = sm; o[3] = n;
  }
}
// folds the partials (device pointer) on the host; out = {min, max, sum}
int stat_finish(const double *d_partial, double out[3], long *n, double *h_pinned = nullptr);   // h_pinned: [STAT_BLOCKS][4] pinned landing block, or a stack copy

}  // namespace hc

namespace hc {
// setExternalVector on part of the domain (cases/kolmogorovFlow/kolmogorovFlow.cpp:136-140): up to HC_MAX_FORCE_REGIONS boxes
// (inclusive global node ranges) whose nodes carry f instead of the uniform body force; a later box overrides an earlier one
struct BodyRegions { int n; int box[HC_MAX_FORCE_REGIONS][6]; double f[HC_MAX_FORCE_REGIONS][3]; };
#ifdef __HIPCC__
__device__ __forceinline__ void region_force(const BodyRegions &r, int xg, int y, int z, double &bx, double &by, double &bz) {
  for (int k = 0; k < r.n; k++) {
    const int *b = r.box[k];
    if (xg >= b[0] && xg <= b[1] && y >= b[2] && y <= b[3] && z >= b[4] && z <= b[5]) { bx = r.f[k][0]; by = r.f[k][1]; bz = r.f[k][2]; }
  }
}

// Zou-He completion on the gathered populations f (stored form f - t_q; the opposite populations of a pair share t_q, so the
// completed ones are formed in that form directly).  With normal x (AXIS 0), code & 3: 0 = velocity 0N, 1 = velocity 0P,
// 2 = pressure 0N, 3 = pressure 0P.  0N completes the five populations with c_x = +1 from their opposites:
//   rho = (S_0 + 2 S_-) / (1 - u_x) with the real sums S (the t_q of the nine c_x = 0 and twice the five c_x = -1 ones add 1),
//   f(1,0,0) = f(-1,0,0) + rho u_x / 3,  f(1,+-1,0) = f(-1,-+1,0) + rho (u_x +- u_y) / 6 -+ N_y,  likewise z,
//   N_y = (sum f over c = (0,1,.) - sum over (0,-1,.)) / 2 - rho u_y / 3;
// 0P mirrors it.  Pressure nodes take rho and u_x = 1 - (S_0 + 2 S_-) / rho (0N), (S_0 + 2 S_+) / rho - 1 (0P), u_y = u_z = 0.
// Normal y (AXIS 1) and z (AXIS 2) are the x completion on swapped populations: axis a exchanges the roles of x and a, so
// population i stands where zh_perm(a, i) -- the direction c_i with those two components exchanged, an involution -- stands
// for x, the normal velocity is u[a] and the tangential pair is (u_x, u_z) for y and (u_y, u_x) for z.  Every sum keeps the
// operand order of the x completion; the indices are template constants, so f stays in registers.
// tests/open_boundary_ref.py restates the x completion operation for operation and tests/open_boundary_axis_ref.py the
// permutation around it.  The collide calls it on fluid nodes before it relaxes, and every observer of an open lattice before
// it takes moments: observe() in lattice.hip (rho_u, pi_neq, plane velocity and pre-inlet coupling, statistics) and
// node_velocity() in ibm.hip.  launch_open() below picks the instantiation that does so, for all of them.
//
// ob_code[node] = -1, or axis << 29 | slot << 2 | kind: the axis sits above the slot, so a node with normal x carries the code
// it always carried and slots stay below 1 << 27 (HC_OB_MAX_SLOTS).
constexpr int HC_OB_AXIS_SHIFT = 29;
constexpr int HC_OB_MAX_SLOTS = 1 << 27;
constexpr int ob_axis(int code) { return code >> HC_OB_AXIS_SHIFT; }
constexpr int ob_slot(int code) { return (code & ((1 << HC_OB_AXIS_SHIFT) - 1)) >> 2; }
constexpr bool ob_is_pressure(int code) { return (code & 2) != 0; }
__host__ __device__ constexpr int zh_perm(int axis, int i) {
  const int x = axis == 1 ? HC_CY[i] : axis == 2 ? HC_CZ[i] : HC_CX[i];
  const int y = axis == 1 ? HC_CX[i] : HC_CY[i];
  const int z = axis == 2 ? HC_CX[i] : HC_CZ[i];
  for (int j = 0; j < HC_Q; j++) if (HC_CX[j] == x && HC_CY[j] == y && HC_CZ[j] == z) return j;
  return -1;
}
template <int AXIS, int I> inline constexpr int ZH = zh_perm(AXIS, I);
static_assert(ZH<0, 7> == 7 && ZH<1, 1> == 2 && ZH<1, 5> == 14 && ZH<1, 15> == 17 && ZH<2, 1> == 3 && ZH<2, 7> == 16 && ZH<2, 13> == 17, "zh_perm");

template <int AXIS>
__device__ __forceinline__ void zou_he(double f[HC_Q], int code, const double *__restrict__ val) {
#define G(I) f[ZH<AXIS, I>]
  const int kind = code & 3;
  const long slot = code >> 2;
  const double s0 = G(0) + G(2) + G(3) + G(8) + G(9) + G(11) + G(12) + G(17) + G(18);
  const double sm = G(1) + G(4) + G(5) + G(6) + G(7);
  const double sp = G(10) + G(13) + G(14) + G(15) + G(16);
  const bool neg = (kind & 1) == 0;   // N
  const double s_out = neg ? sm : sp;
  const double known = s0 + 2.0 * s_out + 1.0;
  double rho, ux, uy, uz;
  if (kind < 2) {
    ux = val[4 * slot + AXIS]; uy = val[4 * slot + (AXIS == 1 ? 0 : 1)]; uz = val[4 * slot + (AXIS == 2 ? 0 : 2)];
    rho = neg ? known / (1.0 - ux) : known / (1.0 + ux);
  } else {
    rho = val[4 * slot + 3];
    ux = neg ? 1.0 - known / rho : known / rho - 1.0;
    uy = 0.0; uz = 0.0;
  }
  const double ny = 0.5 * ((G(11) + G(17) + G(18)) - (G(2) + G(8) + G(9))) - rho * uy / 3.0;
  const double nz = 0.5 * ((G(12) + G(9) + G(17)) - (G(3) + G(8) + G(18))) - rho * uz / 3.0;
  if (neg) {
    G(10) = G(1) + rho * ux / 3.0;
    G(13) = G(4) + rho * (ux + uy) / 6.0 - ny;
    G(14) = G(5) + rho * (ux - uy) / 6.0 + ny;
    G(15) = G(6) + rho * (ux + uz) / 6.0 - nz;
    G(16) = G(7) + rho * (ux - uz) / 6.0 + nz;
  } else {
    G(1) = G(10) - rho * ux / 3.0;
    G(4) = G(13) - rho * (ux + uy) / 6.0 + ny;
    G(5) = G(14) - rho * (ux - uy) / 6.0 - ny;
    G(6) = G(15) - rho * (ux + uz) / 6.0 + nz;
    G(7) = G(16) - rho * (ux - uz) / 6.0 - nz;
  }
#undef G
}

// the completion of an open-boundary node (code >= 0) along the axis its code names; uniform per node
__device__ __forceinline__ void zou_he_node(double f[HC_Q], int code, const double *__restrict__ val) {
  switch (code >> HC_OB_AXIS_SHIFT) {
    case 0: zou_he<0>(f, code, val); break;
    case 1: zou_he<1>(f, code & ((1 << HC_OB_AXIS_SHIFT) - 1), val); break;
    default: zou_he<2>(f, code & ((1 << HC_OB_AXIS_SHIFT) - 1), val); break;
  }
}
#endif
}  // namespace hc

struct hc_lattice {
  int nx, ny, nz;        // local bulk dims
  int periodic[3];       // global periodicity
  int x0, nx_global, n_slabs;
  double omega;
  size_t plane;          // ny*nz nodes of one x-plane
  size_t xs;             // elements from x-plane to x-plane: plane, or plane + 8 rows of padding (see hcl_create)
  size_t npad;           // (nx+2*HALO)*xs
  size_t qstride;        // doubles from population q to q+1 of the same node: npad + padding (see hcl_create)
  hc::DevBuf<double> f[2];   // [19][npad] post-collision populations (fBar), ping-pong
  int cur;               // f[cur] is read by the next collide
  hc::DevBuf<double> force[3];   // [npad][3] IBM force accumulators (a node's three components side by side), rotated: fcur -> (fcur+1)%3 every step
  int fcur;              // force[fcur] is the one spread adds to / collide reads; force[(fcur+2)%3] is the previous
                         // step's (what the interpolation after a collide reads, and what the NEXT collide zeroes);
                         // force[(fcur+1)%3] is already clean, so the spread of the next step may run beside this collide
  int ibm;               // set once membrane cells are bound (hcp_create): collide then reads/zeroes the force buffers
  // dirty map of the IBM force buffers: one byte per group of 16 consecutive nodes (one 128-byte line of a
  // force component) holding the epoch in which spread last touched the group.  The collide kernel reads /
  // zeroes a group only when its byte equals the buffer's current epoch, so untouched lines cost no traffic.
  // Epochs are never cleared (no races); an aliased stale epoch only causes a harmless extra read / zeroing.
  hc::DevBuf<uint8_t> fdirty[3];
  uint8_t fepoch[3];
  // one byte per 8 x 8 x 8 brick of the padded lattice: 1 = the brick holds a non-fluid node or touches a face that stencils
  // cannot cross (the IBM kernels skip the mask look-ups for cells whose tile meets no such brick)
  hc::DevBuf<uint8_t> wallbrick; int nbx, nby, nbz;
  hc::DevBuf<uint8_t> mask;   // [npad]
  std::vector<uint8_t> hmask;  // host copy (cell placement tests against it)
  double body[3];
  hc::BodyRegions regions;   // boxes with their own body force (hcl_set_body_force_regions), global node coordinates
  double wall_u[4][3];   // velocities of the moving-wall mask classes 3..6
  // active-node map of the collide kernel: per padded plane and row, the z-span that holds every node
  // which is not an inert solid, flattened so that a launch only creates threads for those spans
  hc::DevBuf<int> row_z0, row_cum, blk_row;   // [NX*ny], [NX*(ny+1)], [NX*(nblk+1)]
  int nblk, max_active;
  hc::DevBuf<double> scratch;   // download staging
  // slab runs: node velocities u = j/rho + F/2 of the two neighbours' face planes, evaluated there by their owner after the
  // last collide (slab.hip); [side][3][plane].  The interpolation reads them for stencil nodes on the first halo plane
  // instead of gathering 19 populations there.  Valid from the exchange until the next hcl_step_end.
  hc::DevBuf<double> halo_u[2];   // filled and reset by slab.hip
  bool halo_u_valid = false;
  // Lees-Edwards pass (hcl_set_lees_edwards): run after every hcl_step_end of hcl_collide_stream / hc_iterate.  le_D is the
  // current displacement; with le_d != 0, hc_iterate sets it to fmod(le_d * iter, nx) after each step
  bool le_on = false;
  double le_D = 0.0, le_d = 0.0, le_v_top = 0.0, le_v_bottom = 0.0;
  hc::DevBuf<double> le_buf;   // [2][19][nx ny] post-pass values of the top and bottom layers
  // Zou-He open boundaries (hcl_open_boundary_add_axis): ob_code[node] = -1 for every other node, else
  // axis << 29 | slot << 2 | kind (zou_he_node above); ob_val[slot] = {u_x, u_y, u_z, rho} in lattice axes.  The collide runs
  // its open-boundary instantiation while ob_n > 0.
  hc::DevBuf<int> ob_code;          // [npad], device
  std::vector<int> ob_hcode;        // host copy
  hc::DevBuf<double> ob_val;        // [ob_cap][4], device
  int ob_n = 0, ob_cap = 0;
  long ob_epoch = 0;                // counts hcl_open_boundary_clear: a pre-inlet coupling (hc_preinlet) made before one is stale
  // Interior viscosity (hcl_interior_enable): one class byte per node, 0 = omega, k >= 1 = visc_omega[k - 1].  Allocated only
  // once enabled; the collide runs its interior-viscosity instantiation while visc_n > 0.  The passes of interior.hip write it.
  hc::DevBuf<uint8_t> visc_class;   // [npad], device
  int visc_n = 0; double visc_omega[HC_MAX_VISC_CLASSES];
  hc::DevBuf<unsigned long long> visc_vote;   // [npad] scratch of the interior passes: 0 between passes
  // The CEPAC scalar field bound to this lattice (scalar.hip; hcl_scalar_create), or null.  hc_iterate steps it once per
  // iteration.  It does not combine with open boundaries, Lees-Edwards, interior viscosity or a pre-inlet: each of those calls
  // refuses a lattice that has one, and hcl_scalar_create a lattice that has any of them.
  hc_scalar *scalar = nullptr;
  // Solidify mechanics (solidify.hip): the binding field, one byte per node, 1 = a binding site.  Allocated, all 0, by the first
  // hcl_binding_* call.  hcp_solidify_prepare turns fluid nodes into bounce-back nodes and binding sites while a run is
  // queued: it writes mask, binding and wallbrick on the device, and hmask follows at the end of the call that ran it.
  hc::DevBuf<uint8_t> binding;   // [npad], device
  // Running statistics (stats.hip): the one hc_stats bound to this lattice, or null.  hc_iterate samples it at its cadence;
  // hcl_destroy refuses while it is set, so the handle never outlives the lattice.
  hc_stats *stats = nullptr;
  hc::DevBuf<int> ob_list;      // staging of hcl_plane_velocity's node list
  hc::DevBuf<double> ob_out;    // ... and of its output when the caller's buffer is on the host
};

namespace hc {
// The one open-boundary dispatch.  A kernel that observes or advances populations has an OPEN instantiation, which takes the
// plain arguments extended by the open-boundary tables (open_of(L, plain), next to each argument struct) and completes the
// Zou-He nodes; a lattice runs it while it has such nodes and the plain instantiation, as ever, otherwise.
// launch(open, args): open is std::true_type / std::false_type, so that decltype(open)::value is a template argument.
template <class Plain, class Launch>
inline void launch_open(const hc_lattice *L, const Plain &plain, Launch launch) {
  if (L->ob_n > 0) launch(std::true_type{}, open_of(L, plain));
  else launch(std::false_type{}, plain);
}
}  // namespace hc

namespace hc {
int lees_edwards_step(hc_lattice *L);   // lattice.hip: the pass after a step, when enabled
void scalar_lattice_destroyed(hc_lattice *L);   // scalar.hip: hcl_destroy takes the lattice's scalar field with it
// The lattices that live pre-inlet handles (hcl_preinlet_* / hcp_preinlet_*) name, for hcl_scalar_create's refusal.  Kept by
// address in a list of the library's (lattice.hip), not in the lattices: a handle may outlive its lattices, so taking its
// entries out again must not touch them.  `owner` is the handle.
void preinlet_pair_add(const void *owner, const hc_lattice *L);
void preinlet_pair_remove(const void *owner);
void preinlet_pair_forget(const hc_lattice *L);   // hcl_destroy: the address may be handed out again
bool in_preinlet_pair(const hc_lattice *L);
// The lattices whose containers hold a cell type on a three- or four-point IBM kernel (hcp_type_set_ibm_kernel), for the refusals
// of open boundaries and the pre-inlet; kept like the list above.  `owner` is the container, once per wide type.
void ibm_wide_add(const void *owner, const hc_lattice *L);
void ibm_wide_remove_one(const void *owner);   // a type went back to two points
void ibm_wide_remove(const void *owner);       // hcp_destroy
void ibm_wide_forget(const hc_lattice *L);     // hcl_destroy
bool ibm_wide(const hc_lattice *L);
// Running statistics (stats.hip).  stats_fluid_sample (lattice.hip, beside the observers it shares its arithmetic with) queues
// one sample of the fluid sets `what` selects into the accumulator planes; stats_every / stats_sample are what hc_iterate asks
// and does at a sampled iteration; stats_refers_to tells hcp_destroy that a handle still names the container.
int stats_fluid_sample(hc_lattice *L, int what, double *acc_rho_u, double *acc_uu, double *acc_pi, long stride);
int stats_every(const hc_stats *S);
void stats_defer(bool on);   // hc_preinlet_iterate: hc_iterate leaves the due samples to the caller ...
bool stats_deferred();
int stats_sample_if_due(hc_lattice *L, long iterations_done, const char *who);   // ... who takes them here, after its hand-over
int stats_sample(hc_stats *S, const char *who);
bool stats_refers_to(const hc_cells *C);
}

// slab.hip: HemoCell::iterate / collideAndStream on one x-slab of a multi-GPU run (halo and envelope exchange inside)
namespace hcs {
int iterate_slab(hc_lattice *L, hc_cells *C, long *iter, int n, int particle_timescale, int force_limit);
int collide_stream_slab(hc_lattice *L, int nsteps);
void lattice_destroyed(hc_lattice *L);
void halos_stale(hc_lattice *L);   // the populations were replaced from outside: the halo planes have to be fetched again
void set_overlap(int on);
}
