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
// The ray cast itself (raycast.h) is shared with the solidify pass.
#include "raycast.h"

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
    if (ray_crossings(xs, ys, zs, a.tri, a.nt, (double)gx, (double)gy, (double)gz) % 2) atomicMax(&a.vote[node], key);
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
  HC_REQUIRE(C->ibm_kernel[type] == HC_IBM_PHI2, "hcp_type_set_interior_viscosity: the type is on a three- or four-point IBM kernel; the membrane pass walks the eight-node stencil");
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
