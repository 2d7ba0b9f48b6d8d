// Interior viscosity: which lattice nodes lie inside a cell.
//
// Replaces (file:line in the HemoCell tree, INTERIOR_VISCOSITY builds):
//   core/hemoCellParticleField.cpp:777-807   findInternalParticleGridPoints   -> hcp_interior_find
//   helper/octree.h:107-147                  findInnerNodes: bounding box, parity of the ray crossings
//   helper/mollerTrumbore.h                  the ray-triangle test
//   core/hemoCellParticleField.cpp:746-773   internalGridPointsMembrane       -> hcp_interior_membrane
//   mechanics/rbcHighOrderModel.cpp:115-121  the vertex normal the membrane rule reads
//
// Both passes write the lattice's class field (hc_lattice::visc_class), which the interior-viscosity instantiation of the
// collide reads.  One workgroup per cell, vertex positions staged in LDS once.  The reference visits cells and particles one
// after the other and the last writer of a node wins; here every writer first votes with atomicMax on a 64-bit word per node,
//   key = (rank of the cell in ascending (cell id, type) order * widest nv + vertex + 1) << 3 | class   (class 0: clear),
// and a second sweep over the same nodes stores the winner's class and resets the word, so the words are 0 between passes
// and the result is the sequential sweep's whatever the launch geometry.  The ray-cast pass votes per cell (vertex 0).
// Arithmetic follows mollerTrumbore.h and array.h operation for operation (-ffp-contract=off): every decision equals the
// numpy restatement in tests/interior_viscosity_ref.py bit for bit.
#include "cells.h"

namespace {

using u64 = unsigned long long;

struct InteriorArgs {
  LatView v;
  uint8_t *cls;            // [npad] class field
  u64 *vote;               // [npad] vote words, 0 between passes
  int nv, nt, md;
  const int *tri, *vtri;   // [nt][3]; [nv][md] incident triangles, ascending, -1 padded
  const double *px, *py, *pz;   // offset to the type's first vertex
  const int *tag;               // per cell of the type: 0 complete, 1 gone, 2 incomplete
  const unsigned char *dead;    // per vertex of the type
  const int *rank;              // per cell of the type
  long nvmax;                   // widest nv of the marked types
  int klass;
  double area_mean_eq, edge_mean_eq;
  double *normals;              // hcp_interior_normals: [cells * nv][3], else null
};

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { double r = 0.0; r += a0 * b0; r += a1 * b1; r += a2 * b2; return r; }

// hemo::MollerTrumbore (helper/mollerTrumbore.h:30-74) with the ray (-40, -40, -40) from the integer node (ox, oy, oz)
__device__ __forceinline__ int moller_trumbore(double v0x, double v0y, double v0z, double v1x, double v1y, double v1z,
                                               double v2x, double v2y, double v2z, double ox, double oy, double oz) {
  const double EPSILON = 0.0000001;
  const double rx = -40.0, ry = -40.0, rz = -40.0;
  const double e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
  const double e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
  const double px = ry * e2z - rz * e2y, py = rz * e2x - rx * e2z, pz = rx * e2y - ry * e2x;   // crossProduct(rayVector, edge2)
  const double det = dot3(e1x, e1y, e1z, px, py, pz);
  if (det > -EPSILON && det < EPSILON) return 0;
  const double invDet = 1 / det;
  const double sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
  const double u = invDet * dot3(sx, sy, sz, px, py, pz);
  if (u < 0.0 || u > 1.0) return 0;
  const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;   // crossProduct(svec, edge1)
  const double v = invDet * dot3(rx, ry, rz, qx, qy, qz);
  if (v < 0.0 || u + v > 1.0) return 0;
  const float t = (float)(invDet * dot3(e2x, e2y, e2z, qx, qy, qz));   // the reference narrows t to float
  return (double)t > EPSILON ? 1 : 0;
}

// A triangle the exact test can count holds a point Q = node + t (-40, -40, -40) = v0 + u e1 + v e2 up to the rounding of u, v
// and t.  With |det| >= 1e-7, edges up to E and a bounding box up to B lattice units the computed u, v and t are within about
// 1e-6 E B of their real values (numerators of size <= 120 E B carry a few ulps), so Q lies within 3e-6 E^2 B of the
// triangle and, t being > 1e-7 - 1e-6 E B, at most 4e-5 E B above the node on every axis.  CULL_MARGIN = 0.5 lattice units
// covers that for E B up to 1e4 (an RBC at 0.5 um has E B of about 25).  Culled: a triangle whose least x (y, z) exceeds the
// node's by more than the margin, and one whose range of x - y or x - z -- constant along the ray -- excludes the node's by more.
constexpr double CULL_MARGIN = 0.5;

__device__ __forceinline__ double min3(double a, double b, double c) { return fmin(a, fmin(b, c)); }
__device__ __forceinline__ double max3(double a, double b, double c) { return fmax(a, fmax(b, c)); }

// element of the padded lattice of the unwrapped node (gx, gy, gz), by the wrap rules of phi2_stencil, or -1
__device__ __forceinline__ long lattice_node(const LatView &v, long gx, long gy, long gz) {
  long lx = gx - v.x0, ly = gy, lz = gz;
  if (v.wrap_x) lx = pmod(lx, v.nx); else if (lx < 0 || lx >= v.nx) return -1;
  if (gy < 0 || gy >= v.ny) { if (v.per_y) ly = pmod(gy, v.ny); else return -1; }
  if (gz < 0 || gz >= v.nz) { if (v.per_z) lz = pmod(gz, v.nz); else return -1; }
  return (lx + HALO) * (long)v.plane + ly * v.nz + lz;
}

// stages the cell's positions in LDS and returns, to every thread, the truncated bounding box of octree.h:119-121:
// (int)min .. (int)max on every axis.  On a non-periodic axis it is cut to the lattice, which drops only nodes
// lattice_node() drops.
__device__ __forceinline__ void stage_cell(const InteriorArgs &a, double *xs, double *ys, double *zs, int lo[3], int hi[3]) {
  __shared__ double s_red[8][6];
  const int tid = threadIdx.x, nth = blockDim.x, nv = a.nv;
  const long base = (long)blockIdx.x * nv;
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int i = tid; i < nv; i += nth) {
    const double p[3] = {a.px[base + i], a.py[base + i], a.pz[base + i]};
    xs[i] = p[0]; ys[i] = p[1]; zs[i] = p[2];
#pragma unroll
    for (int d = 0; d < 3; d++) { mn[d] = p[d] < mn[d] ? p[d] : mn[d]; mx[d] = p[d] > mx[d] ? p[d] : mx[d]; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const double o = __shfl_xor(mn[d], off), q = __shfl_xor(mx[d], off);
      mn[d] = o < mn[d] ? o : mn[d]; mx[d] = q > mx[d] ? q : mx[d];
    }
  if ((tid & 63) == 0) for (int d = 0; d < 3; d++) { s_red[tid >> 6][d] = mn[d]; s_red[tid >> 6][3 + d] = mx[d]; }
  __syncthreads();
  const int n_ext[3] = {a.v.nx, a.v.ny, a.v.nz};
  const int per[3] = {a.v.wrap_x, a.v.per_y, a.v.per_z};
#pragma unroll
  for (int d = 0; d < 3; d++) {
    double l = s_red[0][d], h = s_red[0][3 + d];
    for (int w = 1; w < (nth + 63) >> 6; w++) { l = s_red[w][d] < l ? s_red[w][d] : l; h = s_red[w][3 + d] > h ? s_red[w][3 + d] : h; }
    // positions far outside the int range (a cell that blew up) are cut before the cast
    l = fmin(fmax(l, -1.0e9), 1.0e9); h = fmin(fmax(h, -1.0e9), 1.0e9);
    lo[d] = (int)l; hi[d] = (int)h;
    if (!per[d]) { const int x0 = d == 0 ? a.v.x0 : 0; lo[d] = lo[d] < x0 ? x0 : lo[d]; hi[d] = hi[d] > x0 + n_ext[d] - 1 ? x0 + n_ext[d] - 1 : hi[d]; }
  }
}

// PHASE 0: vote; PHASE 1: store the winner's class and reset the word
template <int PHASE>
__global__ void interior_find_kernel(InteriorArgs a) {
  extern __shared__ double lds[];
  const int nv = a.nv;
  double *xs = lds, *ys = xs + nv, *zs = ys + nv;
  if (a.tag[blockIdx.x] != 0) return;   // gone, or incomplete (the caller removes those first)
  int lo[3], hi[3];
  stage_cell(a, xs, ys, zs, lo, hi);
  if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) return;
  // a box wider than four periods of a periodic axis belongs to a cell that blew up: it tags nothing, and the sweep stays bounded
  if ((long)hi[0] - lo[0] >= 4L * a.v.nx || (long)hi[1] - lo[1] >= 4L * a.v.ny || (long)hi[2] - lo[2] >= 4L * a.v.nz) return;
  const long ey = (long)hi[1] - lo[1] + 1, ez = (long)hi[2] - lo[2] + 1;
  const long count = ((long)hi[0] - lo[0] + 1) * ey * ez;
  const u64 key = ((u64)((long)a.rank[blockIdx.x] * a.nvmax + 1) << 3) | (u64)a.klass;
  for (long k = threadIdx.x; k < count; k += blockDim.x) {
    const long ix = k / (ey * ez), r = k - ix * ey * ez, iy = r / ez, iz = r - iy * ez;
    const long gx = lo[0] + ix, gy = lo[1] + iy, gz = lo[2] + iz;
    const long node = lattice_node(a.v, gx, gy, gz);
    if (node < 0) continue;
    if (PHASE == 1) {
      const u64 w = a.vote[node];
      if (w) { a.cls[node] = (uint8_t)(w & 7); a.vote[node] = 0; }   // every writer of a node stores the same winner
      continue;
    }
    if (a.v.mask[node] != 0) continue;   // fluid nodes only
    const double ox = (double)gx, oy = (double)gy, oz = (double)gz;
    const double oxy = ox - oy, oxz = ox - oz;
    int crossed = 0;
    for (int t = 0; t < a.nt; t++) {
      const int i0 = a.tri[3 * t], i1 = a.tri[3 * t + 1], i2 = a.tri[3 * t + 2];
      const double v0x = xs[i0], v0y = ys[i0], v0z = zs[i0], v1x = xs[i1], v1y = ys[i1], v1z = zs[i1], v2x = xs[i2], v2y = ys[i2], v2z = zs[i2];
      if (min3(v0x, v1x, v2x) > ox + CULL_MARGIN || min3(v0y, v1y, v2y) > oy + CULL_MARGIN || min3(v0z, v1z, v2z) > oz + CULL_MARGIN) continue;
      const double d0 = v0x - v0y, d1 = v1x - v1y, d2 = v2x - v2y;
      if (min3(d0, d1, d2) > oxy + CULL_MARGIN || max3(d0, d1, d2) < oxy - CULL_MARGIN) continue;
      const double g0 = v0x - v0z, g1 = v1x - v1z, g2 = v2x - v2z;
      if (min3(g0, g1, g2) > oxz + CULL_MARGIN || max3(g0, g1, g2) < oxz - CULL_MARGIN) continue;
      crossed += moller_trumbore(v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, ox, oy, oz);
    }
    if (crossed % 2) atomicMax(&a.vote[node], key);
  }
}

// the normal of vertex i from the LDS positions: sum over its triangles, ascending, of unit normal * (area / area_mean_eq)
// (helper/array.h:270-285, mechanics/rbcHighOrderModel.cpp:117-120)
__device__ __forceinline__ void vertex_normal(const InteriorArgs &a, const double *xs, const double *ys, const double *zs, int i, double n[3]) {
  n[0] = 0.0; n[1] = 0.0; n[2] = 0.0;
  for (int j = 0; j < a.md; j++) {
    const int t = a.vtri[i * a.md + j];
    if (t < 0) break;
    const int i0 = a.tri[3 * t], i1 = a.tri[3 * t + 1], i2 = a.tri[3 * t + 2];
    const double v0x = xs[i0], v0y = ys[i0], v0z = zs[i0];
    const double e1x = xs[i1] - v0x, e1y = ys[i1] - v0y, e1z = zs[i1] - v0z, e2x = xs[i2] - v0x, e2y = ys[i2] - v0y, e2z = zs[i2] - v0z;
    double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    double nn = 0.0; nn += cx * cx; nn += cy * cy; nn += cz * cz; nn = sqrt(nn);
    double area;
    if (nn != 0.0) { area = 0.5 * nn; cx /= nn; cy /= nn; cz /= nn; } else { area = 0.0; cx = cy = cz = 0.0; }
    const double s = area / a.area_mean_eq;
    n[0] += cx * s; n[1] += cy * s; n[2] += cz * s;
  }
}

// PHASE 0: vote; PHASE 1: store and reset; PHASE 2: write the normals (hcp_interior_normals)
template <int PHASE>
__global__ void interior_membrane_kernel(InteriorArgs a) {
  extern __shared__ double lds[];
  const int nv = a.nv;
  double *xs = lds, *ys = xs + nv, *zs = ys + nv;
  const int state = a.tag[blockIdx.x];
  if (state == 1) return;   // the cell is gone
  const long base = (long)blockIdx.x * nv;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) { xs[i] = a.px[base + i]; ys[i] = a.py[base + i]; zs[i] = a.pz[base + i]; }
  __syncthreads();
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    double n[3] = {0.0, 0.0, 0.0};   // an incomplete cell gets no mechanics: its particles keep the zero of the reset
    if (PHASE != 1 && state == 0) vertex_normal(a, xs, ys, zs, i, n);
    if (PHASE == 2) { for (int d = 0; d < 3; d++) a.normals[3 * (base + i) + d] = n[d]; continue; }
    if (a.dead[base + i]) continue;   // a removed particle
    const double p[3] = {xs[i], ys[i], zs[i]};
    Stencil s;
    phi2_stencil(a.v, p[0], p[1], p[2], s);
    long c[3]; int d0[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { c[d] = nearest_node(p[d]); d0[d] = (p[d] < (double)c[d]) ? -1 : 0; }
    const u64 seq = (u64)((long)a.rank[blockIdx.x] * a.nvmax + i + 1) << 3;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {   // the order of phi2_stencil: idx = 4 i + 2 j + k
      const long node = s.node[idx];
      if (node < 0) continue;
      if (PHASE == 1) {
        const u64 w = a.vote[node];
        if (w) { a.cls[node] = (uint8_t)(w & 7); a.vote[node] = 0; }
        continue;
      }
      const double dx = (double)(c[0] + d0[0] + (idx >> 2)) - p[0], dy = (double)(c[1] + d0[1] + ((idx >> 1) & 1)) - p[1],
                   dz = (double)(c[2] + d0[2] + (idx & 1)) - p[2];
      if (sqrt(dx * dx + dy * dy + dz * dz) > a.edge_mean_eq) continue;
      const double dot1 = dot3(dx, dy, dz, n[0], n[1], n[2]);
      atomicMax(&a.vote[node], seq | (u64)(dot1 < 0. ? a.klass : 0));
    }
  }
}

int g_block = 256;

InteriorArgs interior_args(hc_cells *C, int t, const int *d_rank, long nvmax) {
  const hc_celltype *T = C->types[t];
  hc_lattice *L = C->L;
  InteriorArgs a;
  a.v = make_view(L);
  a.cls = L->visc_class; a.vote = L->visc_vote;
  a.nv = T->host.nv; a.nt = T->host.nt; a.md = T->host.md;
  a.tri = T->d_tri; a.vtri = T->d_vtri;
  const TypeArrays va = vert_arrays(C, t);
  a.px = va.p[0]; a.py = va.p[1]; a.pz = va.p[2]; a.tag = va.tag; a.dead = va.dead;
  a.rank = d_rank; a.nvmax = nvmax; a.klass = C->visc_class[t];
  a.area_mean_eq = T->host.area_mean_eq; a.edge_mean_eq = T->host.edge_mean_eq;
  a.normals = nullptr;
  return a;
}

size_t interior_lds(const hc_celltype *T) { return 3 * (size_t)T->host.nv * sizeof(double); }

// Everything a pass needs before its kernels: the vertex arrays on the device, the vote words, and the ranks of the cells of
// the marked types in ascending (cell id, type) order, sorted and staged again only when the ids changed since the last pass.  The host's
// ids are always current (host_cells.h), so this waits for nothing.  off[t]: the type's offset in the rank block.
int prepare(hc_cells *C, const char *who, int **d_rank, long off[8], long *nvmax) {
  hc_lattice *L = C->L;
  if (L->visc_n == 0 || !C->visc_on()) { hc::set_error(std::string(who) + ": no cell type has interior viscosity (hcp_type_set_interior_viscosity)"); return HC_ERR_STATE; }
  int rc = sync_to_device(C); if (rc != HC_OK) return rc;
  if (!L->visc_vote) {
    if ((rc = L->visc_vote.reserve(L->npad)) != HC_OK) return rc;
    HC_HIP(hipMemsetAsync(L->visc_vote, 0, L->npad * sizeof(u64), hc::stream()));
  }
  // the ids of the marked types as the last staging saw them: one comparison per pass, and the sort and the copy below only
  // after cells were appended, compacted, unpacked or a type was marked since
  std::vector<long> seen;
  long n = 0; *nvmax = 1;
  for (int t = 0; t < C->ntypes; t++) {
    off[t] = n;
    if (!C->visc_class[t]) continue;
    HC_REQUIRE(interior_lds(C->types[t]) <= 60 * 1024, std::string(who) + ": the positions of one cell of the type exceed 60 KiB of LDS");
    *nvmax = std::max(*nvmax, (long)C->types[t]->host.nv);
    seen.push_back(-1 - t);   // a separator that no id equals: the same ids split otherwise between two types differ
    seen.insert(seen.end(), C->host[t].ids.begin(), C->host[t].ids.begin() + C->ncells[t]);
    n += C->ncells[t];
  }
  if (seen != C->visc_ids_seen) {
    std::vector<std::array<long, 3>> order;   // id, type, slot
    order.reserve((size_t)n);
    for (int t = 0; t < C->ntypes; t++)
      if (C->visc_class[t]) for (long s = 0; s < C->ncells[t]; s++) order.push_back({C->host[t].ids[(size_t)s], t, s});
    std::sort(order.begin(), order.end());
    std::vector<int> rank((size_t)n);
    for (size_t r = 0; r < order.size(); r++) rank[(size_t)(off[order[r][1]] + order[r][2])] = (int)r;
    int *d = nullptr;
    if ((rc = stage_ints(C->visc_rank, &d, rank.data(), (int)n)) != HC_OK) return rc;
    C->visc_ids_seen.swap(seen);
  }
  *d_rank = C->visc_rank.d;
  return HC_OK;
}

}  // namespace

extern "C" {

int hc_debug_interior_block(int threads) {
  HC_REQUIRE(threads == 64 || threads == 128 || threads == 256 || threads == 512, "hc_debug_interior_block: 64, 128, 256 or 512 threads");
  g_block = threads;
  return HC_OK;
}

int hcp_type_set_interior_viscosity(hc_cells *C, int type, double tau_int) {
  HC_REQUIRE(C && type >= 0 && type < C->ntypes, "hcp_type_set_interior_viscosity: unknown cell type");
  HC_REQUIRE(C->types[type]->host.model == HC_MODEL_RBC_HO, "hcp_type_set_interior_viscosity: interior viscosity needs the vertex normals of HC_MODEL_RBC_HO (RbcHighOrderModel); no other model carries them");
  HC_REQUIRE(tau_int > 0.5, "hcp_type_set_interior_viscosity: tau_int must exceed 0.5");
  hc_lattice *L = C->L;
  const double omega = 1.0 / tau_int;
  // a type is marked once: a second tau_int would leave the first omega behind as a class no type uses, one of the seven
  if (C->visc_class[type]) {
    HC_REQUIRE(L->visc_omega[C->visc_class[type] - 1] == omega, "hcp_type_set_interior_viscosity: the type is marked already with another tau_int");
    return HC_OK;
  }
  int k = 0;
  while (k < L->visc_n && L->visc_omega[k] != omega) k++;
  if (k == L->visc_n) {   // a new class
    HC_REQUIRE(L->visc_n < HC_MAX_VISC_CLASSES, "hcp_type_set_interior_viscosity: more than HC_MAX_VISC_CLASSES distinct interior viscosities");
    double om[HC_MAX_VISC_CLASSES];
    for (int i = 0; i < L->visc_n; i++) om[i] = L->visc_omega[i];
    om[k] = omega;
    const int rc = hcl_interior_enable(L, k + 1, om); if (rc != HC_OK) return rc;
  }
  C->visc_class[type] = k + 1;
  C->visc_ids_seen.clear(); C->visc_ids_seen.push_back(0);   // no list of ids starts with 0: the ranks are formed again
  return HC_OK;
}

int hcp_set_interior_timescales(hc_cells *C, int membrane_every, int entire_grid_every) {
  HC_REQUIRE(C && membrane_every >= 1 && entire_grid_every >= 1, "hcp_set_interior_timescales: timescales must be >= 1");
  C->visc_every = membrane_every; C->visc_grid_every = entire_grid_every;
  return HC_OK;
}

int hcp_interior_find(hc_cells *C) {
  HC_REQUIRE(C, "hcp_interior_find: null pointer");
  int *d_rank; long off[8], nvmax;
  int rc = prepare(C, "hcp_interior_find", &d_rank, off, &nvmax); if (rc != HC_OK) return rc;
  hc_lattice *L = C->L;
  hc::ProfScope prof(hc::PK_INTERIOR_FIND);
  HC_HIP(hipMemsetAsync(L->visc_class, 0, L->npad, hc::stream()));   // "reset all the lattice points" (:779-783)
  for (int phase = 0; phase < 2; phase++)
    for (int t = 0; t < C->ntypes; t++) {
      if (!C->visc_class[t] || C->ncells[t] == 0) continue;
      const InteriorArgs a = interior_args(C, t, d_rank + off[t], nvmax);
      const dim3 grid((unsigned)C->ncells[t]);
      if (phase == 0) hipLaunchKernelGGL(interior_find_kernel<0>, grid, dim3(g_block), interior_lds(C->types[t]), hc::stream(), a);
      else hipLaunchKernelGGL(interior_find_kernel<1>, grid, dim3(g_block), interior_lds(C->types[t]), hc::stream(), a);
      HC_HIP(hipGetLastError());
    }
  return HC_OK;
}

int hcp_interior_membrane(hc_cells *C) {
  HC_REQUIRE(C, "hcp_interior_membrane: null pointer");
  int *d_rank; long off[8], nvmax;
  int rc = prepare(C, "hcp_interior_membrane", &d_rank, off, &nvmax); if (rc != HC_OK) return rc;
  hc::ProfScope prof(hc::PK_INTERIOR_MEMBRANE);
  for (int phase = 0; phase < 2; phase++)
    for (int t = 0; t < C->ntypes; t++) {
      if (!C->visc_class[t] || C->ncells[t] == 0) continue;
      const InteriorArgs a = interior_args(C, t, d_rank + off[t], nvmax);
      const dim3 grid((unsigned)C->ncells[t]);
      if (phase == 0) hipLaunchKernelGGL(interior_membrane_kernel<0>, grid, dim3(g_block), interior_lds(C->types[t]), hc::stream(), a);
      else hipLaunchKernelGGL(interior_membrane_kernel<1>, grid, dim3(g_block), interior_lds(C->types[t]), hc::stream(), a);
      HC_HIP(hipGetLastError());
    }
  return HC_OK;
}

int hcp_interior_normals(hc_cells *C, int type, double *out) {
  HC_REQUIRE(C && out && type >= 0 && type < C->ntypes, "hcp_interior_normals: bad arguments");
  HC_REQUIRE(C->types[type]->host.model == HC_MODEL_RBC_HO, "hcp_interior_normals: only HC_MODEL_RBC_HO carries a vertex normal");
  int rc = settle(C); if (rc != HC_OK) return rc;
  rc = sync_to_device(C); if (rc != HC_OK) return rc;
  const long n = C->ncells[type] * C->types[type]->host.nv;
  if (n == 0) return HC_OK;
  DevBuf<double> d;
  if ((rc = d.reserve((size_t)(3 * n))) != HC_OK) return rc;
  InteriorArgs a = interior_args(C, type, nullptr, 1);
  a.normals = d;
  hipLaunchKernelGGL(interior_membrane_kernel<2>, dim3((unsigned)C->ncells[type]), dim3(g_block), interior_lds(C->types[type]), hc::stream(), a);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(out, d, (size_t)(3 * n) * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));   // before the block is freed
  return HC_OK;
}

}  // extern "C"
