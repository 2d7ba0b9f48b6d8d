// Running statistics on the device: sums of the fluid observables and counts of cell vertices / cell interiors per node,
// sampled at a cadence inside hc_iterate with no host wait.
//
// Replaces, for time-averaged fields, what the reference does offline from its HDF5 output (file:line in the HemoCell tree):
//   io/FluidHdf5IO.hh:374-402    CellDensity: vertices per node, per cell type        -> HC_STATS_CELL_DENSITY
//   helper/octree.h:107-147      findInnerNodes, as the interior-viscosity pass runs it -> HC_STATS_INSIDE (raycast.h, unchanged)
// The fluid sample itself is stats_fluid_kernel in lattice.hip: it shares observe<OPEN>() and the arithmetic of the rho_u and
// pi_neq download kernels, so a sum of samples is a sum of what those downloads report, bit for bit.
//
// Layout.  Fluid sums: 4 + 6 + 6 planes of fp64 in the lattice's PADDED node numbering (the index the populations use), one
// population stride apart -- a wavefront reads and writes 64 consecutive doubles of each plane, whole 128-byte lines, and the
// planes start an odd number of lines apart like the populations (common.h, hcl_create).  A node-major record of 16 doubles
// would be one 128-byte line per lane and 64 lines per wave instruction.  Counts: 64-bit words [type][npad] in the same
// numbering, so lattice_node() of raycast.h indexes them directly; 64 bits cannot wrap, so no sample cap is needed.
#include "raycast.h"
#include <memory>

using u64 = unsigned long long;

struct hc_stats {
  hc_lattice *L = nullptr;
  hc_cells *C = nullptr;
  int what = 0, every = 0, ntypes = 0;
  long samples = 0;
  long stride = 0;                 // doubles between two planes of a fluid set (the population stride of the lattice)
  DevBuf<double> rho_u, uu, pi;    // [4][stride], [6][stride], [6][stride]
  DevBuf<u64> density, inside;     // [ntypes][npad]
  DevBuf<double> stage;            // download staging
};

namespace {

constexpr int FLUID_SETS = HC_STATS_RHO_U | HC_STATS_UU | HC_STATS_PI;
constexpr int CELL_SETS = HC_STATS_CELL_DENSITY | HC_STATS_INSIDE;

std::vector<hc_stats *> g_handles;   // every live handle: hcp_destroy asks by address, without touching a lattice

// +1 at the nearest node of every live vertex of one type (io/FluidHdf5IO.hh:384-396)
__global__ __launch_bounds__(256) void stats_density_kernel(LatView v, long n, const double *px, const double *py, const double *pz, const int *vert_cell,
                                                            const int *tag_all, const unsigned char *dead, u64 *cnt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag_all[vert_cell[i]] == 1) return;   // a removed particle / a cell that is gone
  const long node = lattice_node(v, nearest_node(px[i]), nearest_node(py[i]), nearest_node(pz[i]));
  if (node >= 0) atomicAdd(&cnt[node], 1ULL);
}

struct InsideArgs {
  LatView v;
  int nv, nt;
  const int *tri;
  const double *px, *py, *pz;   // offset to the type's first vertex
  const int *tag;               // per cell of the type
  u64 *cnt;                     // [npad] of the type
};

// +1 on every fluid node the cell's surface encloses; one workgroup per cell, as interior_find_kernel sweeps its box
__global__ void stats_inside_kernel(InsideArgs a) {
  extern __shared__ double lds[];
  const int nv = a.nv;
  double *xs = lds, *ys = xs + nv, *zs = ys + nv;
  if (a.tag[blockIdx.x] != 0) return;   // gone or incomplete: no closed surface
  int lo[3], hi[3];
  stage_cell(a, xs, ys, zs, lo, hi);
  if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) return;
  // a box wider than four periods of an axis belongs to a cell that blew up: it counts nothing, and the sweep stays bounded
  if ((long)hi[0] - lo[0] >= 4L * a.v.nx || (long)hi[1] - lo[1] >= 4L * a.v.ny || (long)hi[2] - lo[2] >= 4L * a.v.nz) return;
  const long ey = (long)hi[1] - lo[1] + 1, ez = (long)hi[2] - lo[2] + 1;
  const long count = ((long)hi[0] - lo[0] + 1) * ey * ez;
  for (long k = threadIdx.x; k < count; k += blockDim.x) {
    const long ix = k / (ey * ez), r = k - ix * ey * ez, iy = r / ez, iz = r - iy * ez;
    const long gx = lo[0] + ix, gy = lo[1] + iy, gz = lo[2] + iz;
    const long node = lattice_node(a.v, gx, gy, gz);
    if (node < 0) continue;
    if (a.v.mask[node] != 0) continue;   // fluid nodes only
    if (ray_crossings(xs, ys, zs, a.tri, a.nt, (double)gx, (double)gy, (double)gz) % 2) atomicAdd(&a.cnt[node], 1ULL);
  }
}

// sums of k planes, padded numbering -> [n][k] in the reference node order
__global__ void stats_gather_fluid_kernel(const double *acc, long stride, int k, int plane, long xs, double *out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= plane) return;
  const int x = blockIdx.y;
  const long node = (long)(x + HALO) * xs + p, o = (long)k * ((long)x * plane + p);
  for (int c = 0; c < k; c++) out[o + c] = acc[(long)c * stride + node];
}

__global__ void stats_gather_counts_kernel(const u64 *cnt, int plane, long xs, long *out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= plane) return;
  const int x = blockIdx.y;
  out[(long)x * plane + p] = (long)cnt[(long)(x + HALO) * xs + p];
}

size_t inside_lds(const hc_celltype *T) { return 3 * (size_t)T->host.nv * sizeof(double); }

int zero(hc_stats *S) {
  if (S->rho_u) HC_HIP(hipMemsetAsync(S->rho_u, 0, 4 * (size_t)S->stride * sizeof(double), hc::stream()));
  if (S->uu) HC_HIP(hipMemsetAsync(S->uu, 0, 6 * (size_t)S->stride * sizeof(double), hc::stream()));
  if (S->pi) HC_HIP(hipMemsetAsync(S->pi, 0, 6 * (size_t)S->stride * sizeof(double), hc::stream()));
  const size_t words = (size_t)S->ntypes * S->L->npad;
  if (S->density) HC_HIP(hipMemsetAsync(S->density, 0, words * sizeof(u64), hc::stream()));
  if (S->inside) HC_HIP(hipMemsetAsync(S->inside, 0, words * sizeof(u64), hc::stream()));
  S->samples = 0;
  return HC_OK;
}

}  // namespace

namespace hc {

int stats_every(const hc_stats *S) { return S->every; }

// hc_preinlet_iterate: an iteration of the coupled pair ends after the fluid hand-over and the cell check, not where the
// domain's own hc_iterate returns.  While deferred, hc_iterate takes no sample itself and the caller takes the due ones at
// its own end of the iteration (stats_sample_if_due), so that a sample there, too, is what the observers would report.
static bool g_deferred = false;
void stats_defer(bool on) { g_deferred = on; }
bool stats_deferred() { return g_deferred; }
int stats_sample_if_due(hc_lattice *L, long iterations_done, const char *who) {
  hc_stats *S = L->stats;
  if (!S || S->every <= 0 || iterations_done % S->every != 0) return HC_OK;
  return stats_sample(S, who);
}

bool stats_refers_to(const hc_cells *C) {
  for (const hc_stats *S : g_handles) if (S->C == C) return true;
  return false;
}

// One sample, queued on the stream in use: the fluid kernel, then per cell type the vertex kernel and the per-cell kernel.
// Nothing here waits for the device or reads the host's view of the cells: the kernels honour the tags and the removed-particle
// flags that the advance kernel keeps on the device.  (sync_to_device copies only when the HOST staging is newer, which inside
// hc_iterate it never is.)
int stats_sample(hc_stats *S, const char *who) {
  hc_lattice *L = S->L;
  int rc;
  if (S->what & FLUID_SETS) {
    hc::ProfScope prof(hc::PK_STATS_FLUID);
    if ((rc = stats_fluid_sample(L, S->what, S->rho_u, S->uu, S->pi, S->stride)) != HC_OK) return rc;
  }
  if (S->what & CELL_SETS) {
    hc_cells *C = S->C;
    if (C->ntypes != S->ntypes) { hc::set_error(std::string(who) + ": cell types were added to the container after hc_stats_create"); return HC_ERR_STATE; }
    if ((rc = sync_to_device(C)) != HC_OK) return rc;
    const LatView v = make_view(L);
    for (int t = 0; t < C->ntypes && C->nverts > 0; t++) {
      const long nc = C->ncells[t], n = nc * C->types[t]->host.nv;
      if (nc == 0) continue;
      const TypeArrays a = vert_arrays(C, t);
      if (S->what & HC_STATS_CELL_DENSITY) {
        hc::ProfScope prof(hc::PK_STATS_DENSITY);
        hipLaunchKernelGGL(stats_density_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, n, (const double *)a.p[0], (const double *)a.p[1],
                           (const double *)a.p[2], a.vert_cell, (const int *)a.tag_all, (const unsigned char *)a.dead, S->density + (size_t)t * L->npad);
        HC_HIP(hipGetLastError());
      }
      if (S->what & HC_STATS_INSIDE) {
        const hc_celltype *T = C->types[t];
        if (inside_lds(T) > 60 * 1024) { hc::set_error(std::string(who) + ": the positions of one cell of a type exceed 60 KiB of LDS"); return HC_ERR_ARG; }
        InsideArgs ia;
        ia.v = v; ia.nv = T->host.nv; ia.nt = T->host.nt; ia.tri = T->d_tri;
        ia.px = a.p[0]; ia.py = a.p[1]; ia.pz = a.p[2]; ia.tag = a.tag; ia.cnt = S->inside + (size_t)t * L->npad;
        hc::ProfScope prof(hc::PK_STATS_INSIDE);
        hipLaunchKernelGGL(stats_inside_kernel, dim3((unsigned)nc), dim3(256), inside_lds(T), hc::stream(), ia);
        HC_HIP(hipGetLastError());
      }
    }
  }
  S->samples++;
  return HC_OK;
}

}  // namespace hc

extern "C" {

int hc_stats_create(hc_lattice *L, hc_cells *C, int what, hc_stats **out) {
  HC_REQUIRE(L && out, "hc_stats_create: null pointer");
  HC_REQUIRE(L->n_slabs == 1, "hc_stats_create: running statistics need the whole domain on one GPU (n_slabs = 1)");
  HC_REQUIRE(!L->stats, "hc_stats_create: the lattice has an hc_stats already");
  HC_REQUIRE(what != 0 && (what & ~(FLUID_SETS | CELL_SETS)) == 0, "hc_stats_create: `what` must be a non-empty mask of the HC_STATS_* sets");
  HC_REQUIRE(!C || C->L == L, "hc_stats_create: the cell container is bound to a different lattice");
  HC_REQUIRE(C || !(what & CELL_SETS), "hc_stats_create: HC_STATS_CELL_DENSITY and HC_STATS_INSIDE need a cell container");
  std::unique_ptr<hc_stats> S(new hc_stats());
  S->L = L; S->C = C; S->what = what; S->stride = (long)L->qstride;
  S->ntypes = (C && (what & CELL_SETS)) ? C->ntypes : 0;
  int rc;
  if ((what & HC_STATS_RHO_U) && (rc = S->rho_u.reserve(4 * (size_t)S->stride)) != HC_OK) return rc;
  if ((what & HC_STATS_UU) && (rc = S->uu.reserve(6 * (size_t)S->stride)) != HC_OK) return rc;
  if ((what & HC_STATS_PI) && (rc = S->pi.reserve(6 * (size_t)S->stride)) != HC_OK) return rc;
  const size_t words = (size_t)(S->ntypes > 0 ? S->ntypes : 1) * L->npad;
  if ((what & HC_STATS_CELL_DENSITY) && (rc = S->density.reserve(words)) != HC_OK) return rc;
  if ((what & HC_STATS_INSIDE) && (rc = S->inside.reserve(words)) != HC_OK) return rc;
  if ((rc = zero(S.get())) != HC_OK) return rc;
  L->stats = S.get();
  g_handles.push_back(S.get());
  *out = S.release();
  return HC_OK;
}

int hc_stats_destroy(hc_stats *S) {
  if (!S) return HC_OK;
  (void)hipStreamSynchronize(hc::stream());   // queued samples still write the sums
  S->L->stats = nullptr;
  g_handles.erase(std::remove(g_handles.begin(), g_handles.end(), S), g_handles.end());
  delete S;
  return HC_OK;
}

int hc_stats_set_every(hc_stats *S, int every) {
  HC_REQUIRE(S, "hc_stats_set_every: null pointer");
  HC_REQUIRE(every >= 0, "hc_stats_set_every: the cadence must be >= 0 (0: explicit samples only)");
  S->every = every;
  return HC_OK;
}

int hc_stats_sample(hc_stats *S) {
  HC_REQUIRE(S, "hc_stats_sample: null pointer");
  return hc::stats_sample(S, "hc_stats_sample");
}

int hc_stats_reset(hc_stats *S) {
  HC_REQUIRE(S, "hc_stats_reset: null pointer");
  return zero(S);
}

int hc_stats_samples(const hc_stats *S, long *n) {
  HC_REQUIRE(S && n, "hc_stats_samples: null pointer");
  *n = S->samples;
  return HC_OK;
}

int hc_stats_download_fluid(hc_stats *S, int set, double *out) {
  HC_REQUIRE(S && out, "hc_stats_download_fluid: null pointer");
  HC_REQUIRE(set == HC_STATS_RHO_U || set == HC_STATS_UU || set == HC_STATS_PI, "hc_stats_download_fluid: `set` must be one of HC_STATS_RHO_U, HC_STATS_UU, HC_STATS_PI");
  HC_REQUIRE(S->what & set, "hc_stats_download_fluid: the set was not selected at hc_stats_create");
  const hc_lattice *L = S->L;
  const int k = set == HC_STATS_RHO_U ? 4 : 6;
  const double *acc = set == HC_STATS_RHO_U ? S->rho_u : set == HC_STATS_UU ? S->uu : S->pi;
  const size_t n = (size_t)L->nx * L->plane;
  HC_HIP(hipStreamSynchronize(hc::stream()));   // the staging block of an earlier download may be replaced
  const int rc = S->stage.reserve(n * 6); if (rc != HC_OK) return rc;
  hipLaunchKernelGGL(stats_gather_fluid_kernel, dim3((unsigned)((L->plane + 255) / 256), (unsigned)L->nx, 1), dim3(256), 0, hc::stream(), acc, S->stride, k,
                     (int)L->plane, (long)L->xs, (double *)S->stage);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(out, S->stage, n * k * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hc_stats_download_cells(hc_stats *S, int set, int type, long *out) {
  HC_REQUIRE(S && out, "hc_stats_download_cells: null pointer");
  HC_REQUIRE(set == HC_STATS_CELL_DENSITY || set == HC_STATS_INSIDE, "hc_stats_download_cells: `set` must be HC_STATS_CELL_DENSITY or HC_STATS_INSIDE");
  HC_REQUIRE(S->what & set, "hc_stats_download_cells: the set was not selected at hc_stats_create");
  HC_REQUIRE(type >= 0 && type < S->ntypes, "hc_stats_download_cells: cell type index out of range");
  const hc_lattice *L = S->L;
  const u64 *cnt = (set == HC_STATS_CELL_DENSITY ? S->density : S->inside) + (size_t)type * L->npad;
  const size_t n = (size_t)L->nx * L->plane;
  HC_HIP(hipStreamSynchronize(hc::stream()));
  const int rc = S->stage.reserve(n * 6); if (rc != HC_OK) return rc;
  static_assert(sizeof(long) == sizeof(double), "the staging block holds either");
  hipLaunchKernelGGL(stats_gather_counts_kernel, dim3((unsigned)((L->plane + 255) / 256), (unsigned)L->nx, 1), dim3(256), 0, hc::stream(), cnt, (int)L->plane,
                     (long)L->xs, reinterpret_cast<long *>(S->stage.p));
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(out, S->stage, n * sizeof(long), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

}  // extern "C"
