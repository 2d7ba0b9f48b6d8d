// Solidify mechanics: platelets that come near a binding site on the wall, under enough shear, turn into wall nodes, and those
// nodes become binding sites themselves (the reference's thrombus-growth model, SOLIDIFY_MECHANICS builds).
//
// Replaces (file:line in the HemoCell tree):
//   core/hemoCellParticleField.cpp:920-948    populateBindingSites              -> hcl_binding_populate
//   core/hemoCellParticleField.cpp:951-1000   eigenValueFromCell (Tresca)       -> hcl_download_tresca, and inside the flag pass
//   mechanics/pltSimpleModel.cpp:211-252      PltSimpleModel::solidifyMechanics -> hcp_solidify_prepare
//   core/hemoCellParticleField.cpp:1018-1065  solidifyCells                     -> hcp_solidify_flag
//   core/hemoCell.cpp:334-340                 the check inside iterate          -> solidify_check (hc_iterate, cells.hip)
//
// State: the binding field (hc_lattice::binding, one byte per node), a flag byte per vertex (hc_cells::d_sflag) and the two
// thresholds of every enabled type.  The prepare pass is the one place where the wall set of a lattice grows while a run is
// queued: it writes the device mask, the binding field and the wall-brick map, all to the value 1, so the result does not depend
// on the launch geometry; the lattice's host mask follows at the end of the call (solidify_refresh_mask).  The new wall
// nodes were fluid, so they lie inside the active spans of the collide and that map stays as it is.
//
// Deviations from the reference: the 26 neighbours of a node wrap on periodic axes and are dropped
// beyond a non-periodic end, where the reference sees them through its envelope; the nearest node of a vertex is
// floor(pos + 0.5), where the reference truncates; vertices of types that are not enabled are never flagged, where the
// reference reads the thresholds of any type and throws where they are missing; the Tresca value of a node that is not fluid
// is 0.
#include "raycast.h"
#include <memory>

namespace {

// ---------------------------------------------------------------------------------------------------------------- binding field
// one thread per node of the (clipped) box: a boundary node with a non-boundary node among its 26 neighbours becomes a site
__global__ __launch_bounds__(256) void binding_populate_kernel(LatView v, uint8_t *binding, int x0, int y0, int z0, int ex, int ey, int ez) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= (long)ex * ey * ez) return;
  const int ix = (int)(k / ((long)ey * ez)), r = (int)(k - (long)ix * ey * ez), iy = r / ez, iz = r - iy * ez;
  const long gx = (long)v.x0 + x0 + ix, gy = y0 + iy, gz = z0 + iz;
  const long node = lattice_node(v, gx, gy, gz);
  if (node < 0 || v.mask[node] == 0) return;
  for (int a = -1; a <= 1; a++)
    for (int b = -1; b <= 1; b++)
      for (int c = -1; c <= 1; c++) {
        const long nb = lattice_node(v, gx + a, gy + b, gz + c);
        if (nb >= 0 && v.mask[nb] == 0) { binding[node] = 1; return; }
      }
}

// ---------------------------------------------------------------------------------------------------------------- Tresca
// One Jacobi rotation that annihilates a_pq of a symmetric 3 x 3 matrix (Rutishauser's form: t = tan of the smaller angle);
// a_rp, a_rq are the two other off-diagonal entries, those of the third row r.
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  double t;
  if (fabs(theta) > 1.0e150) t = 0.5 / theta;   // theta * theta would overflow
  else { t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0)); if (theta < 0.0) t = -t; }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq; aqq = aqq + t * apq; apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
}

// (lambda_max - lambda_min) / 2 of the symmetric matrix (xx, xy, xz, yy, yz, zz).  Cyclic Jacobi with a fixed number of
// sweeps: every eigenvalue comes out to a few roundings of the matrix norm whatever the spectrum, two or three equal
// eigenvalues included, where the closed trigonometric form loses half the digits.  The off-diagonal norm of a 3 x 3 matrix
// falls quadratically after the first sweeps; six sweeps leave it below the rounding of the diagonal for every input.
constexpr int JACOBI_SWEEPS = 6;
__device__ __forceinline__ double tresca_of(double xx, double xy, double xz, double yy, double yz, double zz) {
#pragma unroll 1
  for (int sweep = 0; sweep < JACOBI_SWEEPS; sweep++) {
    jacobi_rotate(xx, yy, xy, xz, yz);   // (p, q) = (0, 1), r = 2
    jacobi_rotate(xx, zz, xz, xy, yz);   // (0, 2), r = 1
    jacobi_rotate(yy, zz, yz, xy, xz);   // (1, 2), r = 0
  }
  const double hi = fmax(xx, fmax(yy, zz)), lo = fmin(xx, fmin(yy, zz));
  return (hi - lo) / 2.0;
}

// eigenValueFromCell on the fluid node `node` = local (lx, ly, lz): PiNeq and rho as the observers of lattice.hip form them
// (pi_neq_kernel, rho_u_kernel; the same gather, the same order of operations), S = -omega * 3 / (2 rho) * PiNeq
__device__ __forceinline__ double tresca_at(const LatView &v, const double *__restrict__ fin, long qs, double omega, int lx, int ly, int lz, long node) {
  double f[HC_Q];
  pull(fin, qs, node, hc::neighbours(v, v.plane, lx, ly, lz), f);
  double rhoBar, j0, j1, j2;
  moments(f, rhoBar, j0, j1, j2);
  const double invRho = 1.0 / (1.0 + rhoBar);
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
  const double pre = (-omega * 3.0) / (2.0 * (1.0 + rhoBar));
  return tresca_of(pre * (xx - invRho * j0 * j0 - cs2 * rhoBar), pre * (xy - invRho * j0 * j1), pre * (xz - invRho * j0 * j2),
                   pre * (yy - invRho * j1 * j1 - cs2 * rhoBar), pre * (yz - invRho * j1 * j2), pre * (zz - invRho * j2 * j2 - cs2 * rhoBar));
}

__global__ __launch_bounds__(256) void tresca_kernel(LatView v, const double *fin, long qs, double omega, double *out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int ny_nz = v.ny * v.nz;
  if (p >= ny_nz) return;
  const int x = blockIdx.y, y = p / v.nz, z = p - y * v.nz;
  const long node = (long)(x + HALO) * v.plane + p;
  out[(long)x * ny_nz + p] = v.mask[node] == 0 ? tresca_at(v, fin, qs, omega, x, y, z, node) : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- prepare
struct PrepareArgs {
  LatView v;
  uint8_t *mask, *binding, *wallbrick;   // written: see the file comment
  int nv, nt;
  const int *tri;                        // [nt][3]
  const double *px, *py, *pz;            // offset to the type's first vertex
  int *tag;                              // per cell of the type
  const unsigned char *sflag;            // per vertex of the type
  int *ntag;                             // hc_cells::d_ntag
  int *solid;                            // hc_cells::d_solid
};

// One workgroup per cell.  A complete cell with a flagged vertex: every fluid node inside it becomes a bounce-back node and a
// binding site, and the cell leaves the way a cell that reached a wall leaves.  The mask byte is set by a 32-bit atomic OR on
// the word that holds it, so that a node inside two such cells is counted once; all other stores are plain byte stores of 1.
// The populations of the node stay as they are.
__global__ void solidify_prepare_kernel(PrepareArgs a) {
  extern __shared__ double lds[];
  __shared__ int s_any;
  const int nv = a.nv;
  double *xs = lds, *ys = xs + nv, *zs = ys + nv;
  if (a.tag[blockIdx.x] != 0) return;   // gone or incomplete (uniform)
  if (threadIdx.x == 0) s_any = 0;
  int lo[3], hi[3];
  stage_cell(a, xs, ys, zs, lo, hi);    // holds a barrier after the store above
  const long base = (long)blockIdx.x * nv;
  bool any = false;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) any = any || a.sflag[base + i] != 0;
  if (any) s_any = 1;
  __syncthreads();
  if (!s_any) return;
  int converted = 0;
  const bool sweep = !(hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) &&
                     // a box wider than four periods of a periodic axis belongs to a cell that blew up: it turns nothing into wall
                     !((long)hi[0] - lo[0] >= 4L * a.v.nx || (long)hi[1] - lo[1] >= 4L * a.v.ny || (long)hi[2] - lo[2] >= 4L * a.v.nz);
  if (sweep) {
    const long ey = (long)hi[1] - lo[1] + 1, ez = (long)hi[2] - lo[2] + 1;
    const long count = ((long)hi[0] - lo[0] + 1) * ey * ez;
    for (long k = threadIdx.x; k < count; k += blockDim.x) {
      const long ix = k / (ey * ez), r = k - ix * ey * ez, iy = r / ez, iz = r - iy * ez;
      const long gx = lo[0] + ix, gy = lo[1] + iy, gz = lo[2] + iz;
      const long node = lattice_node(a.v, gx, gy, gz);
      if (node < 0 || a.mask[node] != 0) continue;   // fluid nodes only
      if (ray_crossings(xs, ys, zs, a.tri, a.nt, (double)gx, (double)gy, (double)gz) % 2 == 0) continue;
      const unsigned bit = 1u << (8 * (unsigned)(node & 3));
      const unsigned old = atomicOr(reinterpret_cast<unsigned *>(a.mask + (node & ~3L)), bit);
      if (((old >> (8 * (unsigned)(node & 3))) & 0xffu) == 0) converted++;
      a.binding[node] = 1;
      const long xp = node / a.v.plane, rem = node - xp * a.v.plane;
      const long y = rem / a.v.nz, z = rem - y * a.v.nz;
      a.wallbrick[((xp >> 3) * a.v.nby + (y >> 3)) * a.v.nbz + (z >> 3)] = 1;
    }
  }
  if (converted) atomicAdd(&a.solid[1], converted);
  if (threadIdx.x == 0 && atomicExch(&a.tag[blockIdx.x], 1) != 1) {
    atomicAdd(&a.ntag[0], 1); atomicAdd(&a.ntag[3], 1);   // gone, and of those the solidified (the compaction's books)
    atomicAdd(&a.solid[0], 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------- flag
// One thread per vertex of an enabled type.  n = the vertex's nearest node; the binding sites among n and its 26 neighbours
// are the sites b of the reference's loop that reach this vertex through node n.  The distance is taken to the unwrapped b.
__global__ __launch_bounds__(256) void solidify_flag_kernel(LatView v, long n, const uint8_t *binding, const double *fin, long qs, double omega,
                                                            const double *px, const double *py, const double *pz, unsigned char *sflag,
                                                            const int *vert_cell, const int *tag, const unsigned char *dead, double dist_max, double shear_min) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (dead[i] || tag[vert_cell[i]] == 1) return;
  const double x = px[i], y = py[i], z = pz[i];
  const long cx = nearest_node(x), cy = nearest_node(y), cz = nearest_node(z);
  const long node = lattice_node(v, cx, cy, cz);
  if (node < 0) return;   // not in the particle grid (update_pg, :158-161)
  bool near = false;
  for (int dx = -1; dx <= 1; dx++)
    for (int dy = -1; dy <= 1; dy++)
      for (int dz = -1; dz <= 1; dz++) {
        const long gx = cx + dx, gy = cy + dy, gz = cz + dz;
        const long b = lattice_node(v, gx, gy, gz);
        if (b < 0 || !binding[b]) continue;
        const double d0 = x - (double)gx, d1 = y - (double)gy, d2 = z - (double)gz;
        if (sqrt(d0 * d0 + d1 * d1 + d2 * d2) <= dist_max) near = true;
      }
  if (!near || v.mask[node] != 0) return;
  const long xp = node / v.plane, rem = node - xp * v.plane;
  const int ly = (int)(rem / v.nz), lz = (int)(rem - (long)ly * v.nz);
  const double tresca = tresca_at(v, fin, qs, omega, (int)xp - HALO, ly, lz, node);
  if (fabs(tresca / 1e-7) > shear_min) sflag[i] = 1;   // 1e-7 is a literal of the reference, not dt
}

// hcl_upload_solidified_mask: every node with add[node] != 0 that is fluid becomes a bounce-back node, as the prepare pass leaves it
__global__ __launch_bounds__(256) void add_walls_kernel(LatView v, long npad, const uint8_t *add, uint8_t *mask, uint8_t *wallbrick) {
  const long node = (long)blockIdx.x * 256 + threadIdx.x;
  if (node >= npad || !add[node] || mask[node] != 0) return;
  mask[node] = 1;
  const long xp = node / v.plane, rem = node - xp * v.plane;
  const long y = rem / v.nz, z = rem - y * v.nz;
  wallbrick[((xp >> 3) * v.nby + (y >> 3)) * v.nbz + (z >> 3)] = 1;
}

__global__ void publish_solid_kernel(const int *solid, int *host_view) { host_view[0] = solid[0]; host_view[1] = solid[1]; }

int g_block = 256;

int ensure_binding(hc_lattice *L) {
  if (L->binding) return HC_OK;
  const int rc = L->binding.reserve(L->npad); if (rc != HC_OK) return rc;
  HC_HIP(hipMemsetAsync(L->binding, 0, L->npad, hc::stream()));
  return HC_OK;
}

// bulk [nx][ny][nz] <-> the padded device numbering
void to_bulk(const hc_lattice *L, const std::vector<uint8_t> &pad, uint8_t *out) {
  for (int x = 0; x < L->nx; x++) std::memcpy(out + (size_t)x * L->plane, pad.data() + (size_t)(x + HALO) * L->xs, L->plane);
}

int refuse(const char *who, const hc_lattice *L) {
  const char *why = solidify_refusal(L);
  if (!why) return HC_OK;
  hc::set_error(std::string(who) + ": " + why);
  return HC_ERR_ARG;
}

}  // namespace

namespace hcc {

const char *solidify_refusal(const hc_lattice *L) {
  if (L->n_slabs > 1) return "solidify mechanics run on one domain (n_slabs = 1)";
  if (L->ob_n > 0) return "solidify mechanics do not combine with open boundaries";
  if (L->le_on) return "solidify mechanics do not combine with a Lees-Edwards boundary";
  if (L->visc_n > 0) return "solidify mechanics do not combine with interior viscosity";
  if (hc::in_preinlet_pair(L)) return "solidify mechanics do not combine with a pre-inlet";
  return nullptr;
}

int ensure_sflag(hc_cells *C) {
  if (C->d_sflag || C->cap <= 0) return HC_OK;
  const int rc = C->d_sflag.reserve((size_t)C->cap); if (rc != HC_OK) return rc;
  HC_HIP(hipMemset(C->d_sflag, 0, (size_t)C->cap));
  return HC_OK;
}

static int launch_prepare(hc_cells *C) {
  hc_lattice *L = C->L;
  hc::ProfScope prof(hc::PK_SOLIDIFY_PREPARE);
  for (int t = 0; t < C->ntypes; t++) {
    if (!C->solid_on[t] || C->ncells[t] == 0) continue;
    const hc_celltype *T = C->types[t];
    const TypeArrays va = vert_arrays(C, t);
    PrepareArgs a;
    a.v = make_view(L);
    a.mask = L->mask; a.binding = L->binding; a.wallbrick = L->wallbrick;
    a.nv = T->host.nv; a.nt = T->host.nt; a.tri = T->d_tri;
    a.px = va.p[0]; a.py = va.p[1]; a.pz = va.p[2]; a.tag = va.tag;
    a.sflag = C->d_sflag + C->first[t];
    a.ntag = C->d_ntag; a.solid = C->d_solid;
    hipLaunchKernelGGL(solidify_prepare_kernel, dim3((unsigned)C->ncells[t]), dim3(g_block), 3 * (size_t)T->host.nv * sizeof(double), hc::stream(), a);
    HC_HIP(hipGetLastError());
  }
  C->maybe_tagged = true;
  return HC_OK;
}

static int launch_flag(hc_cells *C) {
  hc_lattice *L = C->L;
  hc::ProfScope prof(hc::PK_SOLIDIFY_FLAG);
  const LatView v = make_view(L);
  for (int t = 0; t < C->ntypes; t++) {
    const long n = C->ncells[t] * C->types[t]->host.nv;
    if (!C->solid_on[t] || n == 0) continue;
    const TypeArrays a = vert_arrays(C, t);
    hipLaunchKernelGGL(solidify_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), v, n, (const uint8_t *)L->binding,
                       (const double *)L->f[L->cur], (long)L->qstride, L->omega, a.p[0], a.p[1], a.p[2], C->d_sflag + C->first[t], a.vert_cell,
                       (const int *)a.tag_all, (const unsigned char *)a.dead, C->solid_dist[t], C->solid_shear[t]);
    HC_HIP(hipGetLastError());
  }
  return HC_OK;
}

// what both passes need before their kernels; waits for nothing once the arrays exist
static int ready(hc_cells *C, const char *who) {
  if (!C->solidify_on()) { hc::set_error(std::string(who) + ": no cell type has solidify mechanics (hcp_type_set_solidify)"); return HC_ERR_STATE; }
  int rc = refuse(who, C->L); if (rc != HC_OK) return rc;
  if ((rc = sync_to_device(C)) != HC_OK || (rc = ensure_binding(C->L)) != HC_OK) return rc;
  return ensure_sflag(C);
}

int solidify_check(hc_cells *C) {
  int rc = ready(C, "hc_iterate"); if (rc != HC_OK) return rc;
  if (C->nverts == 0) return HC_OK;
  if ((rc = launch_prepare(C)) != HC_OK) return rc;
  return launch_flag(C);
}

int solidify_refresh_mask(hc_cells *C) {
  hc_lattice *L = C->L;
  if (!C->d_solid) return HC_OK;
  hipLaunchKernelGGL(publish_solid_kernel, dim3(1), dim3(1), 0, hc::stream(), (const int *)C->d_solid, C->h_solid.dev);
  HC_HIP(hipGetLastError());
  HC_HIP(hipStreamSynchronize(hc::stream()));
  if ((long)C->h_solid[1] == C->solid_nodes_seen) return HC_OK;
  HC_HIP(hipMemcpy(L->hmask.data(), L->mask, L->npad, hipMemcpyDeviceToHost));
  C->solid_nodes_seen = (long)C->h_solid[1];
  return HC_OK;
}

}  // namespace hcc

extern "C" {

int hc_debug_solidify_block(int threads) {
  HC_REQUIRE(threads == 64 || threads == 128 || threads == 256 || threads == 512, "hc_debug_solidify_block: 64, 128, 256 or 512 threads");
  g_block = threads;
  return HC_OK;
}

int hcl_binding_populate(hc_lattice *L, const int box[6]) {
  HC_REQUIRE(L && box, "hcl_binding_populate: null pointer");
  int rc = refuse("hcl_binding_populate", L); if (rc != HC_OK) return rc;
  if ((rc = ensure_binding(L)) != HC_OK) return rc;
  const int b[6] = {std::max(box[0], 0), std::min(box[1], L->nx - 1), std::max(box[2], 0), std::min(box[3], L->ny - 1), std::max(box[4], 0), std::min(box[5], L->nz - 1)};
  if (b[0] > b[1] || b[2] > b[3] || b[4] > b[5]) return HC_OK;   // nothing of the box lies on the lattice
  const int ex = b[1] - b[0] + 1, ey = b[3] - b[2] + 1, ez = b[5] - b[4] + 1;
  const long n = (long)ex * ey * ez;
  hipLaunchKernelGGL(binding_populate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), make_view(L), L->binding.p, b[0], b[2], b[4], ex, ey, ez);
  HC_HIP(hipGetLastError());
  return HC_OK;
}

int hcl_binding_clear(hc_lattice *L) {
  HC_REQUIRE(L, "hcl_binding_clear: null pointer");
  int rc = refuse("hcl_binding_clear", L); if (rc != HC_OK) return rc;
  if (!L->binding) return ensure_binding(L);
  HC_HIP(hipMemsetAsync(L->binding, 0, L->npad, hc::stream()));
  return HC_OK;
}

int hcl_binding_download(hc_lattice *L, uint8_t *out) {
  HC_REQUIRE(L && out, "hcl_binding_download: null pointer");
  if (!L->binding) { std::memset(out, 0, (size_t)L->nx * L->plane); return HC_OK; }   // never used: no site anywhere
  std::vector<uint8_t> pad(L->npad);
  HC_HIP(hipMemcpyAsync(pad.data(), L->binding, L->npad, hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  to_bulk(L, pad, out);
  return HC_OK;
}

int hcl_binding_upload(hc_lattice *L, const uint8_t *in) {
  HC_REQUIRE(L && in, "hcl_binding_upload: null pointer");
  int rc = refuse("hcl_binding_upload", L); if (rc != HC_OK) return rc;
  if ((rc = ensure_binding(L)) != HC_OK) return rc;
  std::vector<uint8_t> pad(L->npad, 0);
  for (int x = 0; x < L->nx; x++)
    for (size_t p = 0; p < L->plane; p++) pad[(size_t)(x + HALO) * L->xs + p] = in[(size_t)x * L->plane + p] ? 1 : 0;
  HC_HIP(hipMemcpyAsync(L->binding, pad.data(), L->npad, hipMemcpyHostToDevice, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));   // before pad goes
  return HC_OK;
}

int hcl_download_mask(hc_lattice *L, uint8_t *out) {
  HC_REQUIRE(L && out, "hcl_download_mask: null pointer");
  std::vector<uint8_t> pad(L->npad);
  HC_HIP(hipMemcpyAsync(pad.data(), L->mask, L->npad, hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  to_bulk(L, pad, out);
  return HC_OK;
}

int hcl_upload_solidified_mask(hc_lattice *L, const uint8_t *in) {
  HC_REQUIRE(L && in, "hcl_upload_solidified_mask: null pointer");
  int rc = refuse("hcl_upload_solidified_mask", L); if (rc != HC_OK) return rc;
  std::vector<uint8_t> pad(L->npad, 0);
  for (int x = 0; x < L->nx; x++)
    for (size_t p = 0; p < L->plane; p++) pad[(size_t)(x + HALO) * L->xs + p] = in[(size_t)x * L->plane + p] ? 1 : 0;
  hc::DevBuf<uint8_t> d;
  if ((rc = d.reserve(L->npad)) != HC_OK) return rc;
  HC_HIP(hipMemcpyAsync(d, pad.data(), L->npad, hipMemcpyHostToDevice, hc::stream()));
  hipLaunchKernelGGL(add_walls_kernel, dim3((unsigned)((L->npad + 255) / 256)), dim3(256), 0, hc::stream(), make_view(L), (long)L->npad, (const uint8_t *)d.p, L->mask.p, L->wallbrick.p);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(L->hmask.data(), L->mask, L->npad, hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));   // before d and pad go
  return HC_OK;
}

int hcl_download_tresca(hc_lattice *L, double *out) {
  HC_REQUIRE(L && out, "hcl_download_tresca: null pointer");
  HC_REQUIRE(L->n_slabs == 1 && L->ob_n == 0 && L->visc_n == 0, "hcl_download_tresca: one domain without open boundaries and without interior viscosity (the value is formed with the lattice's one omega)");
  const size_t n = (size_t)L->nx * L->plane;
  int rc = L->scratch.reserve(n); if (rc != HC_OK) return rc;
  hipLaunchKernelGGL(tresca_kernel, dim3((unsigned)((L->plane + 255) / 256), (unsigned)L->nx), dim3(256), 0, hc::stream(), make_view(L),
                     (const double *)L->f[L->cur], (long)L->qstride, L->omega, L->scratch.p);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(out, L->scratch, n * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hcp_type_set_solidify(hc_cells *C, int type, double distance_threshold_lu, double shear_threshold) {
  HC_REQUIRE(C && type >= 0 && type < C->ntypes, "hcp_type_set_solidify: unknown cell type");
  HC_REQUIRE(C->types[type]->host.model == HC_MODEL_PLT_SIMPLE, "hcp_type_set_solidify: only HC_MODEL_PLT_SIMPLE (PltSimpleModel) implements solidifyMechanics");
  HC_REQUIRE(distance_threshold_lu >= 0.0 && shear_threshold >= 0.0, "hcp_type_set_solidify: the thresholds must not be negative");   // also refuses NaN
  HC_REQUIRE(3 * (size_t)C->types[type]->host.nv * sizeof(double) <= 60 * 1024, "hcp_type_set_solidify: the positions of one cell of the type exceed 60 KiB of LDS");
  int rc = refuse("hcp_type_set_solidify", C->L); if (rc != HC_OK) return rc;
  if (!C->d_solid) {
    std::unique_ptr<int[]> zero(new int[2]());
    if ((rc = C->d_solid.reserve(2)) != HC_OK || (rc = C->h_solid.reserve(2)) != HC_OK) return rc;
    HC_HIP(hipMemcpy(C->d_solid, zero.get(), 2 * sizeof(int), hipMemcpyHostToDevice));
    C->h_solid[0] = C->h_solid[1] = 0;
  }
  C->solid_on[type] = 1; C->solid_dist[type] = distance_threshold_lu; C->solid_shear[type] = shear_threshold;
  if (!C->host_dirty) return ensure_sflag(C);   // else the next sync_to_device lays the regions out, flags included
  return HC_OK;
}

int hcp_set_solidify_timescale(hc_cells *C, int every) {
  HC_REQUIRE(C && every >= 1, "hcp_set_solidify_timescale: the timescale must be >= 1");
  C->solid_every = every;
  return HC_OK;
}

int hcp_solidify_prepare(hc_cells *C) {
  HC_REQUIRE(C, "hcp_solidify_prepare: null pointer");
  int rc = ready(C, "hcp_solidify_prepare"); if (rc != HC_OK) return rc;
  if (C->nverts > 0 && (rc = launch_prepare(C)) != HC_OK) return rc;
  return solidify_refresh_mask(C);
}

int hcp_solidify_flag(hc_cells *C) {
  HC_REQUIRE(C, "hcp_solidify_flag: null pointer");
  int rc = ready(C, "hcp_solidify_flag"); if (rc != HC_OK) return rc;
  if (C->nverts > 0 && (rc = launch_flag(C)) != HC_OK) return rc;
  return solidify_refresh_mask(C);
}

int hcp_solidify_flags_download(hc_cells *C, unsigned char *out) {
  HC_REQUIRE(C && out, "hcp_solidify_flags_download: null pointer");
  int rc = settle(C); if (rc != HC_OK) return rc;
  rc = sync_to_host(C); if (rc != HC_OK) return rc;
  size_t o = 0;
  for (int t = 0; t < C->ntypes; t++) { const std::vector<unsigned char> &f = C->host[t].sflag; std::copy(f.begin(), f.end(), out + o); o += f.size(); }
  return HC_OK;
}

int hcp_solidify_flags_upload(hc_cells *C, const unsigned char *in) {
  HC_REQUIRE(C && in, "hcp_solidify_flags_upload: null pointer");
  if (!C->solidify_on()) { hc::set_error("hcp_solidify_flags_upload: no cell type has solidify mechanics (hcp_type_set_solidify)"); return HC_ERR_STATE; }
  int rc = settle(C); if (rc != HC_OK) return rc;
  rc = sync_to_host(C); if (rc != HC_OK) return rc;
  size_t o = 0;
  for (int t = 0; t < C->ntypes; t++) {
    std::vector<unsigned char> &f = C->host[t].sflag;
    for (size_t i = 0; i < f.size(); i++) f[i] = in[o + i] ? 1 : 0;
    o += f.size();
  }
  C->host_dirty = true;
  return HC_OK;
}

int hcp_solidify_counts(hc_cells *C, long out[3]) {
  HC_REQUIRE(C && out, "hcp_solidify_counts: null pointer");
  int rc = settle(C); if (rc != HC_OK) return rc;
  rc = sync_to_host(C); if (rc != HC_OK) return rc;
  if ((rc = solidify_refresh_mask(C)) != HC_OK) return rc;   // lands the device counters in h_solid
  out[0] = C->d_solid ? (long)C->h_solid[0] : 0; out[1] = C->d_solid ? (long)C->h_solid[1] : 0; out[2] = 0;
  for (int t = 0; t < C->ntypes; t++) for (unsigned char f : C->host[t].sflag) out[2] += f ? 1 : 0;
  return HC_OK;
}

}  // extern "C"
