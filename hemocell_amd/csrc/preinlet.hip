// The pre-inlet's cells: whole cells found in the pre-inlet's window are copied into the domain, and an outflow sink takes
// cells out of the domain behind a plane.
//
// Replaces (file:line in the HemoCell tree):
//   helper/preInlet.cpp:254-351                                       applyPreInletParticleBoundary
//   core/hemoCellParticleDataTransfer.cpp:33-65, 229-260              the offset of position and cell id
//
// The reference copies single particles; this back end stores cells whole and unwrapped, so a cell is added only when its
// id is absent and its whole vertex set lies in the window.
#include "cells.h"
#include <memory>
#include <set>
#include <unordered_set>
#include <utility>

namespace {

constexpr int SEL = 8;   // doubles per cell slot of the select block: flag, lap, min / max on x, y, z

// One workgroup per cell slot of one type: extents of the live vertices on the three axes, the lap of the cell along `axis`
// (positions are unwrapped: a cell that went k times round the periodic pre-inlet sits at x + k Lp) and whether it lies
// wholly in the window.  fmin / fmax are exact, so the result does not depend on the order of the reduction.
__global__ __launch_bounds__(256) void preinlet_select_kernel(int nv, const double *px, const double *py, const double *pz, const int *tag,
                                                              const unsigned char *dead, int axis, double Lp, double window_lo, double window_hi,
                                                              double *out) {
  __shared__ double red[4][6];
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
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int d = 0; d < 3; d++) { lo[d] = fmin(lo[d], __shfl_xor(lo[d], off)); hi[d] = fmax(hi[d], __shfl_xor(hi[d], off)); }
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
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
    r[0] = (double)flag; r[1] = (double)lap;
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
};

static int axis_nodes(const hc_lattice *L, int axis) { return axis == 0 ? L->nx : axis == 1 ? L->ny : L->nz; }

// room for `total` cell slots in a select block; the old block is given up only once the last check has left it
static int reserve_select(hc_preinlet_cells *X, SelectBlock &b, long total) {
  if ((size_t)(SEL * total) <= b.cap) return HC_OK;
  if (b) HC_HIP(hipEventSynchronize(X->done));
  return b.reserve((size_t)(SEL * (total + total / 4 + 64)));
}

// the select kernel over every type of a container; block row of (type t, slot c) = first[t] + c
static int launch_select(hc_preinlet_cells *X, int which, hc_cells *C, double Lp, double lo, double hi, std::vector<long> &first) {
  first.assign((size_t)C->ntypes + 1, 0);
  for (int t = 0; t < C->ntypes; t++) first[(size_t)t + 1] = first[(size_t)t] + C->ncells[t];
  const long total = first[(size_t)C->ntypes];
  SelectBlock &b = X->sel[which];
  { int rc = reserve_select(X, b, total); if (rc != HC_OK) return rc; }
  for (int t = 0; t < C->ntypes; t++) {
    const long nc = C->ncells[t];
    if (nc == 0) continue;
    const TypeArrays a = vert_arrays(C, t);
    hipLaunchKernelGGL(preinlet_select_kernel, dim3((unsigned)nc), dim3(256), 0, hc::stream(), C->types[t]->host.nv, a.p[0], a.p[1], a.p[2], a.tag, a.dead,
                       X->axis, Lp, lo, hi, b.dev + SEL * first[(size_t)t]);
    HC_HIP(hipGetLastError());
  }
  return HC_OK;
}

extern "C" {

int hcp_preinlet_create(hc_preinlet_cells **out, hc_cells *pre, hc_cells *domain, int axis, int orientation, double window_lo, double window_hi,
                        const double shift[3], long id_stride) {
  HC_REQUIRE(out && pre && domain && shift && pre != domain, "hcp_preinlet_create: bad arguments");
  HC_REQUIRE(axis >= 0 && axis <= 2, "hcp_preinlet_create: axis must be 0, 1 or 2");
  HC_REQUIRE(orientation == -1 || orientation == 1, "hcp_preinlet_create: orientation must be -1 (*neg) or +1 (*pos)");
  HC_REQUIRE(pre->L->n_slabs == 1 && domain->L->n_slabs == 1, "hcp_preinlet_create: needs n_slabs = 1 on both lattices");
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
  hc_cells *both[2] = {pre, domain};
  for (int w = 0; w < 2; w++) {   // the blocks of the cells held now, so that a check allocates only when the cell set has outgrown them
    long total = 0;
    for (int t = 0; t < both[w]->ntypes; t++) total += (long)both[w]->hids[t].size();
    int rc = reserve_select(X.get(), X->sel[w], total); if (rc != HC_OK) return rc;
  }
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
  delete X;
  return HC_OK;
}

int hcp_preinlet_apply(hc_preinlet_cells *X, long *n_injected, long *n_removed) {
  HC_REQUIRE(X, "hcp_preinlet_apply: null handle");
  hc_cells *P = X->pre, *D = X->dom;
  if (n_injected) *n_injected = 0;
  if (n_removed) *n_removed = 0;
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

  // the candidates leave the mapped block before anything below can grow it or move cells
  struct Cand { int slot; long lap; double ext[6]; };
  std::vector<Cand> cand[8];
  for (int t = 0; t < ntypes; t++)
    for (long c = 0; c < P->ncells[t]; c++) {
      const double *r = X->sel[0] + SEL * (pfirst[(size_t)t] + c);
      if (r[0] == 0.0) continue;
      Cand k; k.slot = (int)c; k.lap = (long)r[1];
      for (int e = 0; e < 6; e++) k.ext[e] = r[2 + e];
      cand[t].push_back(k);
    }

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
    const int nv = P->types[t]->host.nv;
    std::unordered_set<long> held(D->hids[t].begin(), D->hids[t].end());
    std::vector<int> src, lap; std::vector<long> ids;
    for (const Cand &k : cand[t]) {
      HC_REQUIRE(k.lap > -(1L << 30) && k.lap < (1L << 30), "hcp_preinlet_apply: lap out of range");
      const long id = P->hids[t][(size_t)k.slot] + (k.lap - X->orient) * X->stride;   // getOffset: positive for *neg
      if (!X->offered.insert(std::make_pair(t, id)).second) continue;
      bool inside = true;
      for (int a = 0; a < 3; a++) {
        const double s = a == X->axis ? X->shift[a] - (double)k.lap * X->Lp : X->shift[a];
        if (k.ext[2 * a] + s < 0.0 || k.ext[2 * a + 1] + s > (double)(axis_nodes(D->L, a) - 1)) inside = false;
      }
      if (!inside) { X->rejected++; continue; }
      if (!held.insert(id).second) continue;
      src.push_back(k.slot); lap.push_back((int)k.lap); ids.push_back(id);
    }
    const int n = (int)ids.size();
    if (n == 0) continue;
    const long slot0 = D->ncells[t];
    if ((rc = append_cells(D, t, ids.data(), nullptr, n, n)) != HC_OK) return rc;   // may move the domain's arrays: taken below
    std::vector<int> lists((size_t)(3 * n));
    for (int i = 0; i < n; i++) { lists[(size_t)i] = src[(size_t)i]; lists[(size_t)(n + i)] = (int)(slot0 + i); lists[(size_t)(2 * n + i)] = lap[(size_t)i]; }
    int *d_lists = nullptr;
    if ((rc = stage_ints(D, 0, &d_lists, lists.data(), 3 * n)) != HC_OK) return rc;
    hipLaunchKernelGGL(preinlet_copy_kernel, dim3((unsigned)n), dim3(256), 0, hc::stream(), nv, n, (const int *)d_lists, vert_arrays(P, t), vert_arrays(D, t),
                       X->axis, X->Lp, X->shift[0], X->shift[1], X->shift[2]);
    HC_HIP(hipGetLastError());
    injected += n;
  }
  X->injected += injected;
  if (n_injected) *n_injected = injected;
  return HC_OK;
}

int hc_preinlet_iterate(hc_preinlet *F, hc_preinlet_cells *X, long *iter, int n, int particle_timescale, int force_limit, int deletion_check_every,
                        int cells_every) {
  HC_REQUIRE(F && X && iter && n >= 0, "hc_preinlet_iterate: bad arguments");
  HC_REQUIRE(cells_every >= 1, "hc_preinlet_iterate: cells_every must be >= 1");
  HC_REQUIRE(particle_timescale >= 1 && deletion_check_every >= 1, "hc_preinlet_iterate: timescales must be >= 1");
  for (int s = 0; s < n; s++) {
    int rc;
    long a = *iter, b = *iter;
    if ((rc = hc_iterate(X->pre->L, X->pre, &a, 1, particle_timescale, force_limit, deletion_check_every)) != HC_OK) return rc;
    if ((rc = hc_iterate(X->dom->L, X->dom, &b, 1, particle_timescale, force_limit, deletion_check_every)) != HC_OK) return rc;
    if ((rc = hcl_preinlet_apply(F)) != HC_OK) return rc;
    *iter = a;
    if (a % cells_every == 0 && (rc = hcp_preinlet_apply(X, nullptr, nullptr)) != HC_OK) return rc;
  }
  return HC_OK;
}

}  // extern "C"
