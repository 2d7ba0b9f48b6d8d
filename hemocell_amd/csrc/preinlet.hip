// The pre-inlet's cells: whole cells found in the pre-inlet's window are copied into the domain, and an outflow sink takes
// cells out of the domain behind a plane.
//
// Replaces (file:line in the HemoCell tree):
//   helper/preInlet.cpp:254-351                                       applyPreInletParticleBoundary
//   core/hemoCellParticleDataTransfer.cpp:33-65, 229-260              the offset of position and cell id
//
// The reference copies single particles; this back end stores cells whole and unwrapped, so a cell is added only when its
// id is absent and its whole vertex set lies in the window.
//
// A domain that is cut into x-slabs takes the same check as a collective (hcp_preinlet_create_slab): the pre-inlet lives whole
// on the rank that holds the inlet plane, the ranks agree over the control plane (hcm::allgatherv) on the cells the sink takes
// and on the candidates whose id some rank holds, and then every rank changes its own container.
#include "cells.h"
#include "comm.h"
#include <memory>
#include <set>
#include <unordered_set>
#include <utility>

namespace {

constexpr int SEL = 8;   // doubles per cell slot of the select block: flag, lap, min / max on x, y, z

// One workgroup per cell slot of one type: extents of the live vertices on the three axes, the lap of the cell along `axis`
// (positions are unwrapped: a cell that went k times round the periodic pre-inlet sits at x + k Lp) and whether it lies
// wholly in the window.  fmin / fmax are exact, so the result does not depend on the order of the reduction.
// SLAB (the sink's select over one x-slab's container): flag and lap give way to the number of live vertices whose nearest node
// lies in the slab [x0, x0 + nx) -- 0 for a pure envelope copy, as in cell_extent_kernel -- and the cell's deletion state.
template <bool SLAB>
__global__ __launch_bounds__(256) void preinlet_select_kernel(int nv, const double *px, const double *py, const double *pz, const int *tag,
                                                              const unsigned char *dead, int axis, double Lp, double window_lo, double window_hi,
                                                              int x0, int nx, double *out) {
  __shared__ double red[4][6];
  __shared__ int red_own[4];
  int own = 0;
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * nv;
  const int state = tag[blockIdx.x];
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  if (state != 1)
    for (int i = tid; i < nv; i += 256) {
      if (dead[base + i]) continue;
      const double x = px[base + i], y = py[base + i], z = pz[base + i];
      lo[0] = fmin(lo[0], x); hi[0] = fmax(hi[0], x);
      lo[1] = fmin(lo[1], y); hi[1] = fmax(hi[1], y);
      lo[2] = fmin(lo[2], z); hi[2] = fmax(hi[2], z);
      if (SLAB) { const long gx = nearest_node(x) - x0; own += (gx >= 0 && gx < nx) ? 1 : 0; }
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int d = 0; d < 3; d++) { lo[d] = fmin(lo[d], __shfl_xor(lo[d], off)); hi[d] = fmax(hi[d], __shfl_xor(hi[d], off)); }
  if (SLAB) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) own += __shfl_xor(own, off);
  }
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    if (SLAB) red_own[w] = own;
#pragma unroll
    for (int d = 0; d < 3; d++) { red[w][2 * d] = lo[d]; red[w][2 * d + 1] = hi[d]; }
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int d = 0; d < 3; d++) {
      lo[d] = fmin(fmin(red[0][2 * d], red[1][2 * d]), fmin(red[2][2 * d], red[3][2 * d]));
      hi[d] = fmax(fmax(red[0][2 * d + 1], red[1][2 * d + 1]), fmax(red[2][2 * d + 1], red[3][2 * d + 1]));
    }
    const double cmin = axis == 0 ? lo[0] : axis == 1 ? lo[1] : lo[2];
    const double cmax = axis == 0 ? hi[0] : axis == 1 ? hi[1] : hi[2];
    long lap = 0; int flag = 0;
    if (state == 0) {   // complete, not gone: every vertex is live
      lap = (long)floor(cmin / Lp);
      flag = (cmin - (double)lap * Lp >= window_lo && cmax - (double)lap * Lp <= window_hi) ? 1 : 0;
    }
    double *r = out + SEL * (long)blockIdx.x;
    if (SLAB) { r[0] = (double)(red_own[0] + red_own[1] + red_own[2] + red_own[3]); r[1] = (double)state; }
    else { r[0] = (double)flag; r[1] = (double)lap; }
    r[2] = lo[0]; r[3] = hi[0]; r[4] = lo[1]; r[5] = hi[1]; r[6] = lo[2]; r[7] = hi[2];
  }
}

// One workgroup per injected cell: the pre-inlet container's slot goes straight into the domain container's slot, shifted.
// lists = [src slot | dst slot | lap] x n.  The envelope counter of unpack_cells_kernel is not touched.
__global__ __launch_bounds__(256) void preinlet_copy_kernel(int nv, int n, const int *lists, VertArrays src, VertArrays dst, int axis, double Lp,
                                                            double shift0, double shift1, double shift2) {
  const int c = blockIdx.x;
  const long s = (long)lists[c] * nv, d = (long)lists[n + c] * nv;
  const double t = (axis == 0 ? shift0 : axis == 1 ? shift1 : shift2) - (double)lists[2 * n + c] * Lp;
  const double t0 = axis == 0 ? t : shift0, t1 = axis == 1 ? t : shift1, t2 = axis == 2 ? t : shift2;
  if (threadIdx.x == 0) dst.tag[lists[n + c]] = 0;
  for (int i = threadIdx.x; i < nv; i += 256) {
    dst.dead[d + i] = 0;
    dst.p[0][d + i] = src.p[0][s + i] + t0; dst.p[1][d + i] = src.p[1][s + i] + t1; dst.p[2][d + i] = src.p[2][s + i] + t2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dst.v[k][d + i] = src.v[k][s + i]; dst.f[k][d + i] = src.f[k][s + i];
      if (dst.r[k]) dst.r[k][d + i] = src.r[k] ? src.r[k][s + i] : 0.0;
    }
  }
}

using SelectBlock = MappedBuf<double>;   // mapped pinned block the select kernel writes, SEL doubles per cell, all types of one container back to back

}  // namespace

struct hc_preinlet_cells {
  hc_cells *pre, *dom;        // not owned: the handle is destroyed before either container
  int axis, orient;
  double lo, hi, shift[3], Lp;
  long stride;
  int sink_on = 0; double sink_plane = 0.0;
  long injected = 0, rejected = 0, removed = 0, checks = 0;
  std::set<std::pair<int, long>> offered;   // (type, id') already offered to the domain
  SelectBlock sel[2];
  Event done;
  bool slab = false;          // hcp_preinlet_create_slab: dom is one x-slab, pre is null off the rank that holds the inlet plane
};

static int axis_nodes(const hc_lattice *L, int axis) { return axis == 0 ? L->nx : axis == 1 ? L->ny : L->nz; }
static int global_nodes(const hc_lattice *L, int axis) { return axis == 0 ? L->nx_global : axis_nodes(L, axis); }

// room for `total` cell slots in a select block; the old block is given up only once the last check has left it
static int reserve_select(hc_preinlet_cells *X, SelectBlock &b, long total) {
  if ((size_t)(SEL * total) <= b.cap) return HC_OK;
  if (b) HC_HIP(hipEventSynchronize(X->done));
  return b.reserve((size_t)(SEL * (total + total / 4 + 64)));
}

// the select kernel over every type of a container; block row of (type t, slot c) = first[t] + c
// (slab: the instantiation that counts the vertices this slab owns)
static int launch_select(hc_preinlet_cells *X, int which, hc_cells *C, double Lp, double lo, double hi, std::vector<long> &first, bool slab = false) {
  first.assign((size_t)C->ntypes + 1, 0);
  for (int t = 0; t < C->ntypes; t++) first[(size_t)t + 1] = first[(size_t)t] + C->ncells[t];
  const long total = first[(size_t)C->ntypes];
  SelectBlock &b = X->sel[which];
  { int rc = reserve_select(X, b, total); if (rc != HC_OK) return rc; }
  for (int t = 0; t < C->ntypes; t++) {
    const long nc = C->ncells[t];
    if (nc == 0) continue;
    const TypeArrays a = vert_arrays(C, t);
    hipLaunchKernelGGL(slab ? preinlet_select_kernel<true> : preinlet_select_kernel<false>, dim3((unsigned)nc), dim3(256), 0, hc::stream(), C->types[t]->host.nv,
                       a.p[0], a.p[1], a.p[2], a.tag, a.dead, X->axis, Lp, lo, hi, C->L->x0, C->L->nx, b.dev + SEL * first[(size_t)t]);
    HC_HIP(hipGetLastError());
  }
  return HC_OK;
}

// what create and create_slab ask of the two containers and the window
static int check_pair(const std::string &fn, const hc_cells *pre, const hc_cells *domain, int axis, double window_lo, double window_hi, long id_stride) {
  HC_REQUIRE(pre->L->periodic[axis], fn + ": the pre-inlet must be periodic on the inlet axis");
  HC_REQUIRE(pre->ntypes == domain->ntypes, fn + ": the containers hold different numbers of cell types");
  for (int t = 0; t < pre->ntypes; t++) {
    const CellTables &a = pre->types[t]->host, &b = domain->types[t]->host;
    HC_REQUIRE(a.model == b.model && a.nv == b.nv, fn + ": the cell types differ in model or vertices");
  }
  HC_REQUIRE(pre->rep_on() == domain->rep_on(), fn + ": repulsion is enabled on one container only");
  HC_REQUIRE(window_lo >= 0.0 && window_hi <= (double)axis_nodes(pre->L, axis) && window_hi > window_lo, fn + ": the window must satisfy 0 <= lo < hi <= Lp");
  HC_REQUIRE(id_stride > 0, fn + ": id_stride must be positive");
  return HC_OK;
}

// the blocks of the cells held now, so that a check allocates only when the cell set has outgrown them
static int reserve_blocks(hc_preinlet_cells *X) {
  hc_cells *both[2] = {X->pre, X->dom};
  for (int w = 0; w < 2; w++) {
    if (!both[w]) continue;
    long total = 0;
    for (int t = 0; t < both[w]->ntypes; t++) total += (long)both[w]->host[t].cells();
    int rc = reserve_select(X, X->sel[w], total); if (rc != HC_OK) return rc;
  }
  return HC_OK;
}

struct Cand { int slot; long lap; double ext[6]; };

// the candidates of the pre-inlet's select leave the mapped block before anything can grow it or move cells
static void take_candidates(const hc_preinlet_cells *X, const std::vector<long> &pfirst, std::vector<Cand> cand[8]) {
  const hc_cells *P = X->pre;
  for (int t = 0; t < P->ntypes; t++)
    for (long c = 0; c < P->ncells[t]; c++) {
      const double *r = X->sel[0] + SEL * (pfirst[(size_t)t] + c);
      if (r[0] == 0.0) continue;
      Cand k; k.slot = (int)c; k.lap = (long)r[1];
      for (int e = 0; e < 6; e++) k.ext[e] = r[2 + e];
      cand[t].push_back(k);
    }
}

// do the shifted extents of a candidate lie in the box [0, n - 1] of the whole domain on every axis?
static bool arrives_inside(const hc_preinlet_cells *X, const Cand &k) {
  for (int a = 0; a < 3; a++) {
    const double s = a == X->axis ? X->shift[a] - (double)k.lap * X->Lp : X->shift[a];
    if (k.ext[2 * a] + s < 0.0 || k.ext[2 * a + 1] + s > (double)((X->slab ? global_nodes(X->dom->L, a) : axis_nodes(X->dom->L, a)) - 1)) return false;
  }
  return true;
}

// n cells of type t of the pre-inlet (slots src, laps lap) join the end of the domain's region with the ids given and are
// copied slot to slot
static int copy_in(hc_preinlet_cells *X, int t, const std::vector<int> &src, const std::vector<int> &lap, const std::vector<long> &ids) {
  hc_cells *P = X->pre, *D = X->dom;
  const int n = (int)ids.size();
  if (n == 0) return HC_OK;
  int rc;
  const long slot0 = D->ncells[t];
  if ((rc = append_cells(D, t, ids.data(), nullptr, n, n)) != HC_OK) return rc;   // may move the domain's arrays: taken below
  std::vector<int> lists((size_t)(3 * n));
  for (int i = 0; i < n; i++) { lists[(size_t)i] = src[(size_t)i]; lists[(size_t)(n + i)] = (int)(slot0 + i); lists[(size_t)(2 * n + i)] = lap[(size_t)i]; }
  int *d_lists = nullptr;
  if ((rc = stage_ints(D, 0, &d_lists, lists.data(), 3 * n)) != HC_OK) return rc;
  hipLaunchKernelGGL(preinlet_copy_kernel, dim3((unsigned)n), dim3(256), 0, hc::stream(), P->types[t]->host.nv, n, (const int *)d_lists, vert_arrays(P, t),
                     vert_arrays(D, t), X->axis, X->Lp, X->shift[0], X->shift[1], X->shift[2]);
  HC_HIP(hipGetLastError());
  return HC_OK;
}

// ---------------------------------------------------------------------------- the check on x-slabs
// One control-plane round of a collective call.  Every rank contributes its return code so far, its error text when that code
// is not HC_OK, and a payload of longs, so a rank that failed locally still completes the round.  When any rank failed, every
// rank returns the first failing rank's code (the others with that rank's message): nobody is left waiting in a collective.
static int agree(const char *fn, int rc, const std::vector<long> &mine, std::vector<std::vector<long>> &all) {
  const std::string why = rc != HC_OK ? std::string(hc_last_error()) : std::string();
  std::vector<long> block{(long)rc, (long)mine.size(), (long)why.size()};
  block.insert(block.end(), mine.begin(), mine.end());
  block.resize(block.size() + (why.size() + sizeof(long) - 1) / sizeof(long), 0L);
  if (!why.empty()) std::memcpy(block.data() + 3 + mine.size(), why.data(), why.size());
  std::vector<std::vector<char>> raw;
  { const int e = hcm::allgatherv(block.data(), block.size() * sizeof(long), raw); if (e != HC_OK) return e; }
  all.assign(raw.size(), std::vector<long>());
  int bad = -1, bad_rc = HC_OK; std::string bad_why;
  for (size_t r = 0; r < raw.size(); r++) {
    const size_t n = raw[r].size() / sizeof(long);
    std::vector<long> b(n);
    if (n) std::memcpy(b.data(), raw[r].data(), n * sizeof(long));
    if (n < 3 || b[1] < 0 || b[2] < 0 || 3 + (size_t)b[1] + ((size_t)b[2] + sizeof(long) - 1) / sizeof(long) != n) { hc::set_error(std::string(fn) + ": corrupt block from rank " + std::to_string(r)); return HC_ERR_STATE; }
    if (b[0] != HC_OK && bad < 0) { bad = (int)r; bad_rc = (int)b[0]; bad_why.assign(reinterpret_cast<const char *>(b.data() + 3 + b[1]), (size_t)b[2]); }
    all[r].assign(b.begin() + 3, b.begin() + 3 + b[1]);
  }
  if (bad < 0) return HC_OK;
  if (bad != hcm::rank()) hc::set_error(std::string(fn) + ": rank " + std::to_string(bad) + " failed: " + bad_why);
  else hc::set_error(bad_why);
  return bad_rc;
}

static long bits_of(double v) { long b; std::memcpy(&b, &v, sizeof(b)); return b; }

using IdSet = std::set<std::pair<int, long>>;   // (type, cell id)

// hcp_preinlet_apply on a slab handle.  Nothing of the domain changes before the last round is over, so an error on any rank
// leaves every container as it was.
static int apply_slab(hc_preinlet_cells *X, long *n_injected, long *n_removed) {
  static const char *fn = "hcp_preinlet_apply";
  hc_cells *P = X->pre, *D = X->dom;
  const int ntypes = D->ntypes;
  std::vector<long> pfirst, dfirst;
  std::vector<Cand> cand[8];
  std::vector<std::pair<int, int>> offer;   // (type, index into cand[type]) of the candidates announced, in ascending (type, slot) order
  std::vector<std::vector<char>> past((size_t)ntypes);   // per held cell: it reaches past the sink plane
  bool selected = false;
  IdSet offers;   // what this check offers for the first time; remembered once the check is through

  // round 1: [sink on, plane, rejected, n sink pairs, n candidate pairs | (type, id) of the cells this rank owns part of and sees
  // past the plane | (type, id') of the candidates]
  std::vector<long> mine{(long)X->sink_on, bits_of(X->sink_plane), 0, 0, 0};
  auto first_part = [&]() -> int {
    int rc;
    if ((P && (rc = settle(P)) != HC_OK) || (rc = settle(D)) != HC_OK) return rc;
    if ((P && (rc = sync_to_device(P)) != HC_OK) || (rc = sync_to_device(D)) != HC_OK) return rc;
    HC_REQUIRE(!P || P->ntypes == ntypes, std::string(fn) + ": the containers no longer hold the same cell types");
    if (P && (rc = launch_select(X, 0, P, X->Lp, X->lo, X->hi, pfirst)) != HC_OK) return rc;
    selected = X->sink_on && D->nverts > 0;
    if (selected && (rc = launch_select(X, 1, D, (double)D->L->nx_global, 0.0, 0.0, dfirst, true)) != HC_OK) return rc;
    HC_HIP(hipEventRecord(X->done, hc::stream()));
    HC_HIP(hipEventSynchronize(X->done));   // the one wait of a check
    std::vector<long> sunk, offered;
    if (selected)
      for (int t = 0; t < ntypes; t++) {
        past[(size_t)t].assign((size_t)D->ncells[t], 0);
        for (long c = 0; c < D->ncells[t]; c++) {
          const double *r = X->sel[1] + SEL * (dfirst[(size_t)t] + c);
          const double cmin = r[2], cmax = r[3];
          if (cmin > cmax) continue;   // no live vertex
          if (!(X->orient < 0 ? cmax > X->sink_plane : cmin < X->sink_plane)) continue;
          past[(size_t)t][(size_t)c] = 1;
          if (r[0] > 0.0) { sunk.push_back(t); sunk.push_back(D->host[t].ids[(size_t)c]); }   // a pure copy is its owners' business
        }
      }
    if (P) {
      take_candidates(X, pfirst, cand);
      for (int t = 0; t < ntypes; t++)
        for (size_t i = 0; i < cand[t].size(); i++) {
          const Cand &k = cand[t][i];
          HC_REQUIRE(k.lap > -(1L << 30) && k.lap < (1L << 30), std::string(fn) + ": lap out of range");
          const long id = P->host[t].ids[(size_t)k.slot] + (k.lap - X->orient) * X->stride;
          if (X->offered.count(std::make_pair(t, id)) || !offers.insert(std::make_pair(t, id)).second) continue;
          if (!arrives_inside(X, k)) { mine[2]++; continue; }
          offer.push_back(std::make_pair(t, (int)i)); offered.push_back(t); offered.push_back(id);
        }
    }
    mine[3] = (long)(sunk.size() / 2); mine[4] = (long)(offered.size() / 2);
    mine.insert(mine.end(), sunk.begin(), sunk.end());
    mine.insert(mine.end(), offered.begin(), offered.end());
    return HC_OK;
  };
  std::vector<std::vector<long>> all;
  int rc = agree(fn, first_part(), mine, all);
  if (rc != HC_OK) return rc;

  // what every rank reads out of round 1, in rank order
  IdSet sunk;
  std::vector<std::pair<int, long>> announced;
  long rejected = 0;
  for (const std::vector<long> &b : all) {
    if (b.size() < 5 || b[3] < 0 || b[4] < 0 || (size_t)(5 + 2 * b[3] + 2 * b[4]) != b.size() || b[0] != all[0][0] || b[1] != all[0][1]) {
      hc::set_error(std::string(fn) + ": the ranks disagree about the sink (hcp_preinlet_set_sink is called with the same arguments on every rank)");
      return HC_ERR_STATE;   // read from the same blocks on every rank: they all return here
    }
    rejected += b[2];
    for (long i = 0; i < b[3]; i++) sunk.insert(std::make_pair((int)b[5 + 2 * i], b[6 + 2 * i]));
    for (long i = 0; i < b[4]; i++) announced.push_back(std::make_pair((int)b[5 + 2 * b[3] + 2 * i], b[6 + 2 * b[3] + 2 * i]));
  }
  // the handle's books change only once every rank is through the last round: a check that failed has offered nothing
  auto through = [&]() { X->checks++; X->rejected += rejected; X->offered.insert(offers.begin(), offers.end()); };
  if (!all[0][0] && announced.empty()) { through(); return HC_OK; }   // no sink and nothing offered: one round

  // round 2: [(type, id') of the candidates this rank will still hold once the sink has run].  A holder checks the sink's list
  // against its own select first: a cell some rank takes out and another keeps would be an orphan.
  std::vector<long> held;
  auto second_part = [&]() -> int {
    for (int t = 0; t < ntypes && selected; t++)
      for (long c = 0; c < D->ncells[t]; c++) {
        const long id = D->host[t].ids[(size_t)c];
        if ((past[(size_t)t][(size_t)c] != 0) != (sunk.count(std::make_pair(t, id)) != 0)) {
          hc::set_error(std::string(fn) + ": this rank's copy of cell " + std::to_string(id) + " of type " + std::to_string(t) +
                        " and its owners disagree on whether it lies past the sink plane");
          return HC_ERR_STATE;
        }
      }
    for (const std::pair<int, long> &a : announced) {
      if (a.first < 0 || a.first >= ntypes || sunk.count(a)) continue;
      const std::vector<long> &ids = D->host[a.first].ids;
      if (std::find(ids.begin(), ids.end(), a.second) != ids.end()) { held.push_back(a.first); held.push_back(a.second); }
    }
    return HC_OK;
  };
  rc = agree(fn, second_part(), held, all);
  if (rc != HC_OK) return rc;
  through();
  IdSet taken;
  for (const std::vector<long> &b : all) for (size_t i = 0; i + 1 < b.size(); i += 2) taken.insert(std::make_pair((int)b[i], b[i + 1]));

  // the sink: every holder, owners and pure copies alike
  for (int t = 0; t < ntypes && !sunk.empty(); t++) {
    std::vector<int> gone;
    for (long c = 0; c < D->ncells[t]; c++) if (sunk.count(std::make_pair(t, D->host[t].ids[(size_t)c]))) gone.push_back((int)c);
    if (gone.empty()) continue;
    if ((rc = hcp_remove_cells(D, t, gone.data(), (int)gone.size())) != HC_OK) return rc;
    D->ext_pending[t] = false;   // extents on their way to the next envelope synchronisation describe the old slots
  }
  X->removed += (long)sunk.size();
  if (n_removed) *n_removed = (long)sunk.size();

  // the injection: a candidate arrives when no rank holds its id and no earlier candidate of this check took it
  long injected = 0;
  std::vector<int> src[8], lap[8]; std::vector<long> ids[8];
  for (size_t i = 0; i < announced.size(); i++) {
    if (!taken.insert(announced[i]).second) continue;
    injected++;
    if (!P) continue;
    const int t = offer[i].first; const Cand &k = cand[t][(size_t)offer[i].second];
    src[t].push_back(k.slot); lap[t].push_back((int)k.lap); ids[t].push_back(announced[i].second);
  }
  for (int t = 0; t < ntypes && P; t++) {
    if (ids[t].empty()) continue;
    if ((rc = copy_in(X, t, src[t], lap[t], ids[t])) != HC_OK) return rc;
    D->ext_pending[t] = false;
  }
  X->injected += injected;
  if (n_injected) *n_injected = injected;
  return HC_OK;
}

extern "C" {

int hcp_preinlet_create(hc_preinlet_cells **out, hc_cells *pre, hc_cells *domain, int axis, int orientation, double window_lo, double window_hi,
                        const double shift[3], long id_stride) {
  HC_REQUIRE(out && pre && domain && shift && pre != domain, "hcp_preinlet_create: bad arguments");
  HC_REQUIRE(axis >= 0 && axis <= 2, "hcp_preinlet_create: axis must be 0, 1 or 2");
  HC_REQUIRE(orientation == -1 || orientation == 1, "hcp_preinlet_create: orientation must be -1 (*neg) or +1 (*pos)");
  HC_REQUIRE(pre->L->n_slabs == 1 && domain->L->n_slabs == 1, "hcp_preinlet_create: needs n_slabs = 1 on both lattices");
  HC_REQUIRE(!pre->L->scalar && !domain->L->scalar, "hcp_preinlet_create: a lattice has a scalar field; the scalar field and a pre-inlet do not combine");
  HC_REQUIRE(!hc::ibm_wide(pre->L) && !hc::ibm_wide(domain->L), "hcp_preinlet_create: a cell type of a lattice is on a three- or four-point IBM kernel; those and a pre-inlet do not combine");
  HC_REQUIRE(pre->L->periodic[axis], "hcp_preinlet_create: the pre-inlet must be periodic on the inlet axis");
  HC_REQUIRE(pre->ntypes == domain->ntypes, "hcp_preinlet_create: the containers hold different numbers of cell types");
  for (int t = 0; t < pre->ntypes; t++) {
    const CellTables &a = pre->types[t]->host, &b = domain->types[t]->host;
    HC_REQUIRE(a.model == b.model && a.nv == b.nv, "hcp_preinlet_create: the cell types differ in model or vertices");
  }
  HC_REQUIRE(pre->rep_on() == domain->rep_on(), "hcp_preinlet_create: repulsion is enabled on one container only");
  const double Lp = (double)axis_nodes(pre->L, axis);
  HC_REQUIRE(window_lo >= 0.0 && window_hi <= Lp && window_hi > window_lo, "hcp_preinlet_create: the window must satisfy 0 <= lo < hi <= Lp");
  HC_REQUIRE(id_stride > 0, "hcp_preinlet_create: id_stride must be positive");
  if (hc::stream() == nullptr) { hc::set_error("hcp_preinlet_create: hc_init() has not been called"); return HC_ERR_STATE; }
  std::unique_ptr<hc_preinlet_cells> X(new hc_preinlet_cells());
  X->pre = pre; X->dom = domain; X->axis = axis; X->orient = orientation; X->lo = window_lo; X->hi = window_hi; X->Lp = Lp; X->stride = id_stride;
  for (int d = 0; d < 3; d++) X->shift[d] = shift[d];
  { const int rc = X->done.create(); if (rc != HC_OK) return rc; }
  { const int rc = reserve_blocks(X.get()); if (rc != HC_OK) return rc; }
  hc::preinlet_pair_add(X.get(), pre->L); hc::preinlet_pair_add(X.get(), domain->L);
  *out = X.release();
  return HC_OK;
}

int hcp_preinlet_create_slab(hc_preinlet_cells **out, hc_cells *pre, hc_cells *domain, int axis, int orientation, double window_lo, double window_hi,
                             const double shift[3], long id_stride) {
  static const std::string fn = "hcp_preinlet_create_slab";
  HC_REQUIRE(out && domain && shift, fn + ": bad arguments");
  const hc_lattice *L = domain->L;
  HC_REQUIRE(L->n_slabs > 1 && hcm::active() && hcm::world() == L->n_slabs,
             fn + ": the domain must be one x-slab of a connected world, one rank per slab (hcp_preinlet_create couples a whole domain)");
  if (hc::stream() == nullptr) { hc::set_error(fn + ": hc_init() has not been called"); return HC_ERR_STATE; }
  // from here on the call is collective: a rank that refuses its arguments says so in the round, and every rank returns
  auto local = [&]() -> int {
    HC_REQUIRE(axis == 0, fn + ": only axis 0 feeds a slab (Xneg on rank 0, Xpos on the last rank)");
    HC_REQUIRE(orientation == -1 || orientation == 1, fn + ": orientation must be -1 (Xneg) or +1 (Xpos)");
    HC_REQUIRE(!L->periodic[0], fn + ": a slab domain that is periodic along x has no inlet plane");
    const bool inlet = orientation < 0 ? L->x0 == 0 : L->x0 + L->nx == L->nx_global;
    HC_REQUIRE(inlet || !pre, fn + ": pre must be null on a rank that does not hold the inlet plane");
    HC_REQUIRE(!inlet || pre, fn + ": the rank that holds the inlet plane needs the pre-inlet's container");
    HC_REQUIRE(id_stride > 0, fn + ": id_stride must be positive");
    if (!pre) return HC_OK;
    HC_REQUIRE(pre != domain && pre->L->n_slabs == 1, fn + ": the pre-inlet needs n_slabs = 1 (it lives whole on the inlet rank)");
    HC_REQUIRE(!pre->L->scalar, fn + ": the pre-inlet's lattice has a scalar field; the scalar field and a pre-inlet do not combine");
    HC_REQUIRE(!hc::ibm_wide(pre->L), fn + ": a cell type of the pre-inlet's lattice is on a three- or four-point IBM kernel; those and a pre-inlet do not combine");
    { const int rc = check_pair(fn, pre, domain, axis, window_lo, window_hi, id_stride); if (rc != HC_OK) return rc; }
    // an arriving cell is held by this rank alone until the ordinary envelope synchronisation replicates it
    const double a = window_lo + shift[0], b = window_hi + shift[0], x0 = (double)L->x0, x1 = (double)(L->x0 + L->nx), e = domain->e_share;
    HC_REQUIRE(orientation < 0 ? (a >= x0 && b <= x1 - e) : (a >= x0 + e && b <= x1),
               fn + ": the window's image [" + std::to_string(a) + ", " + std::to_string(b) + "] must lie in the inlet rank's slab [" + std::to_string(x0) + ", " +
                   std::to_string(x1) + "] at least the particle envelope (" + std::to_string(e) + " lu) away from its inner face");
    return HC_OK;
  };
  std::vector<long> mine{(long)axis, (long)orientation, bits_of(window_lo), bits_of(window_hi), bits_of(shift[0]), bits_of(shift[1]), bits_of(shift[2]), id_stride,
                         (long)domain->ntypes};
  std::vector<std::vector<long>> all;
  { const int rc = agree(fn.c_str(), local(), mine, all); if (rc != HC_OK) return rc; }
  for (const std::vector<long> &b : all) HC_REQUIRE(b == all[0], fn + ": the ranks passed different arguments");
  std::unique_ptr<hc_preinlet_cells> X(new hc_preinlet_cells());
  X->pre = pre; X->dom = domain; X->axis = axis; X->orient = orientation; X->lo = window_lo; X->hi = window_hi; X->stride = id_stride; X->slab = true;
  X->Lp = pre ? (double)axis_nodes(pre->L, axis) : 0.0;
  for (int d = 0; d < 3; d++) X->shift[d] = shift[d];
  { const int rc = X->done.create(); if (rc != HC_OK) return rc; }
  { const int rc = reserve_blocks(X.get()); if (rc != HC_OK) return rc; }
  if (pre) hc::preinlet_pair_add(X.get(), pre->L);
  hc::preinlet_pair_add(X.get(), domain->L);
  *out = X.release();
  return HC_OK;
}

int hcp_preinlet_set_sink(hc_preinlet_cells *X, int on, double plane) {
  HC_REQUIRE(X, "hcp_preinlet_set_sink: null handle");
  X->sink_on = on != 0; X->sink_plane = plane;
  return HC_OK;
}

int hcp_preinlet_counts(const hc_preinlet_cells *X, long out[4]) {
  HC_REQUIRE(X && out, "hcp_preinlet_counts: null pointer");
  out[0] = X->injected; out[1] = X->rejected; out[2] = X->removed; out[3] = X->checks;
  return HC_OK;
}

int hcp_preinlet_destroy(hc_preinlet_cells *X) {
  if (!X) return HC_OK;
  (void)hipStreamSynchronize(hc::stream());
  hc::preinlet_pair_remove(X);
  delete X;
  return HC_OK;
}

int hcp_preinlet_apply(hc_preinlet_cells *X, long *n_injected, long *n_removed) {
  HC_REQUIRE(X, "hcp_preinlet_apply: null handle");
  hc_cells *P = X->pre, *D = X->dom;
  if (n_injected) *n_injected = 0;
  if (n_removed) *n_removed = 0;
  if (X->slab) return apply_slab(X, n_injected, n_removed);
  int rc;
  if ((rc = settle(P)) != HC_OK || (rc = settle(D)) != HC_OK) return rc;
  if ((rc = sync_to_device(P)) != HC_OK || (rc = sync_to_device(D)) != HC_OK) return rc;
  HC_REQUIRE(P->ntypes == D->ntypes, "hcp_preinlet_apply: the containers no longer hold the same cell types");
  const int ntypes = P->ntypes;
  std::vector<long> pfirst, dfirst;
  if ((rc = launch_select(X, 0, P, X->Lp, X->lo, X->hi, pfirst)) != HC_OK) return rc;
  const bool sink = X->sink_on && D->nverts > 0;
  if (sink && (rc = launch_select(X, 1, D, (double)axis_nodes(D->L, X->axis), 0.0, 0.0, dfirst)) != HC_OK) return rc;
  HC_HIP(hipEventRecord(X->done, hc::stream()));
  HC_HIP(hipEventSynchronize(X->done));   // the one wait of a check: for the select kernels, not for the device
  X->checks++;

  std::vector<Cand> cand[8];
  take_candidates(X, pfirst, cand);

  // the sink: cells of the domain that reach past the plane, downstream of it
  if (sink) {
    long removed = 0;
    for (int t = 0; t < ntypes; t++) {
      std::vector<int> gone;
      for (long c = 0; c < D->ncells[t]; c++) {
        const double *r = X->sel[1] + SEL * (dfirst[(size_t)t] + c);
        const double cmin = r[2 + 2 * X->axis], cmax = r[3 + 2 * X->axis];
        if (cmin > cmax) continue;   // no live vertex
        if (X->orient < 0 ? cmax > X->sink_plane : cmin < X->sink_plane) gone.push_back((int)c);
      }
      if (gone.empty()) continue;
      if ((rc = hcp_remove_cells(D, t, gone.data(), (int)gone.size())) != HC_OK) return rc;
      removed += (long)gone.size();
    }
    X->removed += removed;
    if (n_removed) *n_removed = removed;
  }

  // the injection, candidates in ascending (type, slot) order
  long injected = 0;
  for (int t = 0; t < ntypes; t++) {
    if (cand[t].empty()) continue;
    std::unordered_set<long> held(D->host[t].ids.begin(), D->host[t].ids.end());
    std::vector<int> src, lap; std::vector<long> ids;
    for (const Cand &k : cand[t]) {
      HC_REQUIRE(k.lap > -(1L << 30) && k.lap < (1L << 30), "hcp_preinlet_apply: lap out of range");
      const long id = P->host[t].ids[(size_t)k.slot] + (k.lap - X->orient) * X->stride;   // getOffset: positive for *neg
      if (!X->offered.insert(std::make_pair(t, id)).second) continue;
      if (!arrives_inside(X, k)) { X->rejected++; continue; }
      if (!held.insert(id).second) continue;
      src.push_back(k.slot); lap.push_back((int)k.lap); ids.push_back(id);
    }
    if ((rc = copy_in(X, t, src, lap, ids)) != HC_OK) return rc;
    injected += (long)ids.size();
  }
  X->injected += injected;
  if (n_injected) *n_injected = injected;
  return HC_OK;
}

int hc_preinlet_iterate(hc_preinlet *F, hc_preinlet_cells *X, long *iter, int n, int particle_timescale, int force_limit, int deletion_check_every,
                        int cells_every) {
  HC_REQUIRE(X && iter && n >= 0, "hc_preinlet_iterate: bad arguments");
  // a slab handle on a rank without the inlet plane has neither a pre-inlet nor a fluid coupling: that rank steps its slab
  HC_REQUIRE((F != nullptr) == (X->pre != nullptr), "hc_preinlet_iterate: bad arguments (the fluid handle is null exactly on the ranks of a slab handle that hold no pre-inlet)");
  HC_REQUIRE(cells_every >= 1, "hc_preinlet_iterate: cells_every must be >= 1");
  HC_REQUIRE(particle_timescale >= 1 && deletion_check_every >= 1, "hc_preinlet_iterate: timescales must be >= 1");
  // an injected cell would arrive with untagged nodes inside it, and the pre-inlet's own field is not built
  HC_REQUIRE(X->dom->L->visc_n == 0 && !(X->pre && X->pre->L->visc_n), "hc_preinlet_iterate: a lattice has interior viscosity enabled; interior viscosity and a pre-inlet do not combine");
  // Running statistics: a lattice that carries an hc_stats is sampled at the end of the coupled iteration, after the hand-over
  // and the cell check, which is where this call would return -- not where the lattice's own hc_iterate does.  Without a
  // handle on either lattice nothing changes and nothing is launched.
  const bool stats = X->dom->L->stats || (X->pre && X->pre->L->stats);
  struct Defer { bool on; explicit Defer(bool o) : on(o) { if (on) hc::stats_defer(true); } ~Defer() { if (on) hc::stats_defer(false); } } defer(stats);
  for (int s = 0; s < n; s++) {
    int rc;
    long a = *iter, b = *iter;
    if (X->pre && (rc = hc_iterate(X->pre->L, X->pre, &a, 1, particle_timescale, force_limit, deletion_check_every)) != HC_OK) return rc;
    if ((rc = hc_iterate(X->dom->L, X->dom, &b, 1, particle_timescale, force_limit, deletion_check_every)) != HC_OK) return rc;
    if (F && (rc = hcl_preinlet_apply(F)) != HC_OK) return rc;
    *iter = b;
    if (b % cells_every == 0 && (rc = hcp_preinlet_apply(X, nullptr, nullptr)) != HC_OK) return rc;
    if (stats) {
      if (X->pre && (rc = hc::stats_sample_if_due(X->pre->L, b, "hc_preinlet_iterate")) != HC_OK) return rc;
      if ((rc = hc::stats_sample_if_due(X->dom->L, b, "hc_preinlet_iterate")) != HC_OK) return rc;
    }
  }
  return HC_OK;
}

}  // extern "C"
