// Internal declarations shared by the translation units that work on membrane vertices
// (cells.hip: storage and stepping, ibm.hip: spread / interpolate with two-, three- and four-point delta
// functions, mechanics.hip: membrane models,
// exchange.hip: slab envelopes and statistics, repulsion.hip: vertex-vertex and boundary repulsion,
// preinlet.hip: cell injection and the outflow sink, solidify.hip: binding sites and solidification).
//
// Layout (HBM): vertices are a structure of arrays pos/vel/frc[3][n], cell major (a cell's nv vertices are
// contiguous, cells of one type contiguous in a fixed-capacity region), so a wavefront touches 64 consecutive
// doubles per component and a mechanics workgroup stages one whole cell in LDS with coalesced loads.
#pragma once
#include "common.h"
#include "host_cells.h"
#include "mesh.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace hc;

struct hc_celltype {
  CellTables host;
  DevBuf<int> d_tri, d_edge, d_ebt, d_ebo, d_iedge, d_vtri, d_vtri_k, d_vedge, d_vedge_s, d_bsrc, d_vouter, d_vinner, d_vinner_s, d_ring, d_nring;
  DevBuf<double> d_tri_area_eq, d_edge_len_eq, d_edge_angle_eq, d_patch_eq, d_iedge_len_eq;
};

struct hc_cells {
  hc_lattice *L = nullptr;
  hc_params P;
  int ntypes = 0;
  hc_celltype *types[8];
  int timescale[8];
  HostCells host[8];             // host staging per type: ids always current, the payload only while the host holds it (host_cells.h)
  bool host_dirty = false;       // host staging newer than device
  long nverts = 0, cap = 0;      // live vertices (all types); allocated vertex capacity
  long ncells[8] = {0};
  long capc[8] = {0};            // per-type capacity in cells (device regions are fixed-size per type)
  long first[8] = {0};           // first vertex of each type's region on the device
  long cell0[8] = {0};           // first cell slot of each type's region
  DevBuf<double> pos[3], vel[3], frc[3];   // [cap]
  // Deletion lives on the device (core/hemoCellParticleField.cpp:566-588, :304-321 without a host round trip):
  // d_tag per cell slot: 0 complete, 1 gone (every kernel skips the cell; the slot is reclaimed at the next
  // compaction), 2 incomplete (the reference's state after removeParticles(1) took single particles out: no
  // mechanics, forces zeroed at the next material step, the remaining particles are still spread / interpolated /
  // advanced); d_vdead per vertex: 1 = removed particle.
  DevBuf<int> d_tag;             // [tag_cap] all types, slot order
  long tag_cap = 0;
  DevBuf<unsigned char> d_vdead; // [cap]
  MappedBuf<int> h_ntag;         // pinned host copy of the counters {cells gone and not yet compacted, cells made incomplete}; .dev: its device view
  DevBuf<int> d_ntag;            // device counters [2]
  Event ntag_ev;                 // completion of an asynchronous counter read (hc_iterate polls it, never waits)
  bool ntag_pending = false, maybe_tagged = false;
  int del_mode = HC_DELETE_PARTICLE;
  DevBuf<int> d_vert_cell;       // [cap] cell slot of every vertex
  // vertex-vertex repulsion (core/hemoCellParticleField.cpp:677-743); arrays exist only once it is enabled
  DevBuf<double> rep[3];
  int rep_enabled = 0, rep_timescale = 1; double rep_const = 0, rep_cutoff = 0;
  // boundary particles (core/hemoCellParticleField.cpp:865-918): flag map of the wall nodes that repel vertices
  int brep_enabled = 0, brep_timescale = 1; double brep_const = 0, brep_cutoff = 0; DevBuf<uint8_t> d_bflag;
  bool rep_on() const { return rep_enabled || brep_enabled; }
  DevBuf<unsigned int> d_keys[2]; DevBuf<int> d_vals[2]; DevBuf<char> d_sort_tmp; long sort_cap = 0;
  // staged slot lists (envelope exchange, interpolate_cells, remove): pinned host block -> device block, stream ordered;
  // the event guards the pinned block against being rewritten while its copy is still in flight
  // staged slot lists: 0, 1 envelope exchange; 2 reproducible spread; 3 + 2 * type + half: the two halves of a slab's velocity update
  Staged<int> iscratch[19];
  // asynchronous cell extents (hcp_cell_extents_begin / _end): mapped pinned block [4 * cells] the kernel writes, and event, per type
  MappedBuf<double> h_ext[8]; long ext_n[8] = {0}; Event ext_done[8]; bool ext_pending[8] = {false};
  // staging of hcp_add_vertex_force (called every iteration by the stretch drivers): pinned host block + device block
  // [n indices | 3n force components], grown on demand; the event guards the pinned block against reuse in flight
  Staged<char> vf;
  // reproducible spread (hc_set_reproducible_spread): (node, entry) pairs of every (particle, stencil node), both sort buffers,
  // and the three force components of every entry
  DevBuf<unsigned int> det_keys[2]; DevBuf<int> det_vals[2]; DevBuf<double> det_val[3]; DevBuf<char> det_tmp; long det_cap = 0;
  Staged<double> stat;   // [STAT_BLOCKS][4] partials of the statistics reductions, device and pinned host
  Staged<double> info;   // scratch of the information calls (hcp_cell_info, hcp_mechanics_components, statistics)
  // slab runs: ids of cells this rank compacted away on its own (a host query between two envelope synchronisations:
  // counts, output, deleteIncompleteCells) -- the next synchronisation tells the other holders, or their copy would come
  // back as a fresh complete cell
  std::vector<long> slab_gone[8];
  // slab runs: a cell that reaches within e_share lattice units of a face is replicated on the neighbour (the cell-granular
  // form of the reference's particle envelope, core/hemoCell.cpp:139; hcp_set_envelope).  env_viol counts the copies that
  // arrived too late -- a particle already sat on the receiving slab's side when its cell first got there (mapped pinned
  // memory, written by unpack_cells_kernel)
  double e_share = 4.0;
  MappedBuf<int> h_env_viol;
  std::vector<long> slab_rejected;   // (type, cell id) pairs hcp_add_cell rejected at a wall on this slab, until hcp_slab_sync_placement
  // interior viscosity (interior.hip): the lattice class of each type (0: the type is not marked), the cadences of the two
  // passes inside hc_iterate, and the rank of every cell of the marked types in ascending (cell id, type) order -- [type's
  // offset + slot], formed and staged again only when the ids changed
  int visc_class[8] = {0};
  int visc_every = 1, visc_grid_every = 1;
  Staged<int> visc_rank; std::vector<long> visc_ids_seen;   // the ids (per marked type, behind a separator) the staged ranks were formed from
  bool visc_on() const { for (int t = 0; t < ntypes; t++) if (visc_class[t]) return true; return false; }
  // solidify mechanics (solidify.hip): per type the two thresholds of its <MaterialModel> (solid_on[t] = 0: the type takes no
  // part), the cadence of the check inside hc_iterate, and a one-byte flag per vertex that exists once a type is enabled and
  // travels with the cells through the host staging (HostCells::sflag).  d_solid = {cells solidified, nodes solidified} since
  // the container was made, counted on the device; h_solid is where solidify_refresh_mask reads them, and solid_nodes_seen the
  // node count the lattice's host mask was last refreshed at.  A solidified cell also counts in d_ntag[0] and d_ntag[3], so
  // that the compaction takes it out and n_deleted leaves it out.
  int solid_on[8] = {0}; double solid_dist[8] = {0}, solid_shear[8] = {0};
  int solid_every = 1;
  DevBuf<unsigned char> d_sflag;   // [cap]
  DevBuf<int> d_solid; MappedBuf<int> h_solid;
  long solid_nodes_seen = 0;
  bool solidify_on() const { for (int t = 0; t < ntypes; t++) if (solid_on[t]) return true; return false; }
  // width of the IBM delta function per type (hcp_type_set_ibm_kernel): the stencil policy the kernels of ibm.hip are launched
  // with.  hc::ibm_wide(L) knows the lattices that have a type on HC_IBM_PHI3 or HC_IBM_PHI4.
  int ibm_kernel[8] = {HC_IBM_PHI2, HC_IBM_PHI2, HC_IBM_PHI2, HC_IBM_PHI2, HC_IBM_PHI2, HC_IBM_PHI2, HC_IBM_PHI2, HC_IBM_PHI2};
  bool ibm_wide_on() const { for (int t = 0; t < ntypes; t++) if (ibm_kernel[t] != HC_IBM_PHI2) return true; return false; }
  long n_deleted = 0;              // cells removed entirely (by a wall or by the caller; solidified cells are counted apart)
  long n_particles_deleted = 0;    // single particles removed (reference mode), including those of cells removed later
};

namespace hcc {

constexpr double E_SHARE_DEFAULT = 4.0, E_SHARE_MIN = 2.0;   // slab runs, hc_cells::e_share: default, and the least that still covers the IBM stencil

// ----------------------------------------------------------------------------
// lattice view for the IBM kernels
struct LatView {
  const uint8_t *mask;
  int nx, ny, nz; long plane; long npad;   // plane: elements from x-plane to x-plane (hc_lattice::xs)
  int x0;                 // global x of local plane 0
  int wrap_x, halo_x;     // single periodic slab: wrap; multi slab: one halo plane is addressable
  int per_y, per_z;
  int nx_global;
  uint8_t *dirty; uint8_t epoch;   // dirty map of the force buffer spread adds to (see common.h)
  const uint8_t *wallbrick; int nby, nbz;   // wall proximity per 8^3 brick (see common.h)
  const double *halo_u[2];                  // slab runs: owner-evaluated node velocities of the first halo planes (null: gather them here)
  int ny_nz;                                // nodes of one x-plane (stride of the three components of halo_u)
};

inline LatView make_view(const hc_lattice *L) {
  LatView v;
  v.mask = L->mask; v.nx = L->nx; v.ny = L->ny; v.nz = L->nz; v.plane = (long)L->xs; v.npad = (long)L->npad;
  v.x0 = L->x0; v.wrap_x = (L->n_slabs == 1 && L->periodic[0]) ? 1 : 0; v.halo_x = L->n_slabs > 1 ? 1 : 0;
  v.per_y = L->periodic[1]; v.per_z = L->periodic[2]; v.nx_global = L->nx_global;
  v.dirty = L->fdirty[L->fcur]; v.epoch = L->fepoch[L->fcur];
  v.wallbrick = L->wallbrick; v.nby = L->nby; v.nbz = L->nbz;
  v.halo_u[0] = L->halo_u_valid ? L->halo_u[0] : nullptr; v.halo_u[1] = L->halo_u_valid ? L->halo_u[1] : nullptr; v.ny_nz = (int)L->plane;
  return v;
}

__device__ __forceinline__ long pmod(long a, long n) { long r = a % n; return r < 0 ? r + n : r; }

// phi2 (core/immersedBoundaryMethod.h:37-41)
__device__ __forceinline__ double phi2(double x) { x = fabs(x); x = 1.0 - x; return x > 0.0 ? x : 0.0; }

struct Stencil {
  long node[8];     // padded-lattice element index, -1 when not admitted
  double w[8];      // normalised weights
  int lx[8], ly[8], lz[8];  // local (wrapped) coordinates of the node, for the population gather
};

// interpolationCoefficientsPhi2 (core/immersedBoundaryMethod.h:62-138).  Per axis only the pair
// {centre-1, centre} (x < centre) or {centre, centre+1} can carry a non-zero tent weight, and visiting
// the 2x2x2 pairs in ascending offset order is the reference's 27-node loop with its zero-weight skips.
__device__ __forceinline__ long nearest_node(double x) { return (long)floor(x + 0.5); }

__device__ __forceinline__ void phi2_stencil(const LatView &v, double px, double py, double pz, Stencil &s) {
  // weights are formed in GLOBAL coordinates (identical bits on every slab that holds a copy of the
  // vertex); only the node index is made slab-local.  plint(x+0.5) of the reference (:86) truncates,
  // which equals floor on the block-relative coordinates (>= 0) it is applied to; floor is used so that
  // a periodic image at negative x picks the same nodes as its wrapped position.
  const double p[3] = {px, py, pz};
  long c[3]; int d0[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { c[a] = nearest_node(p[a]); d0[a] = (p[a] < (double)c[a]) ? -1 : 0; }
  double total = 0.0;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int idx = i * 4 + j * 2 + k;
        const long gx = c[0] + d0[0] + i, gy = c[1] + d0[1] + j, gz = c[2] + d0[2] + k;
        long lx = gx - v.x0, ly = gy, lz = gz;
        bool ok = true;
        if (v.wrap_x) lx = pmod(lx, v.nx);
        else if (v.halo_x) ok = ok && (lx >= -HALO && lx < v.nx + HALO);
        else ok = ok && (lx >= 0 && lx < v.nx);
        if (gy < 0 || gy >= v.ny) { if (v.per_y) ly = pmod(gy, v.ny); else ok = false; }
        if (gz < 0 || gz >= v.nz) { if (v.per_z) lz = pmod(gz, v.nz); else ok = false; }
        double weight = 0.0; long node = -1;
        if (ok) {
          weight = phi2(p[0] - (double)gx) * phi2(p[1] - (double)gy) * phi2(p[2] - (double)gz);
          if (weight != 0.0) {
            node = (lx + HALO) * (long)v.plane + ly * v.nz + lz;
            if (v.mask[node] != 0) node = -1;
          }
        }
        if (node >= 0) total += weight;
        s.node[idx] = node; s.w[idx] = weight; s.lx[idx] = (int)lx; s.ly[idx] = (int)ly; s.lz[idx] = (int)lz;
      }
  const double coeff = 1.0 / total;
#pragma unroll
  for (int idx = 0; idx < 8; idx++) s.w[idx] *= coeff;
}

struct VertArrays { double *p[3], *v[3], *f[3], *r[3]; unsigned char *dead; int *tag; };   // r: repulsion force arrays or null; dead / tag offset to the type
// what a launch site takes for one type (vert_arrays): the kernel argument above, and the two pointers of the per-vertex
// kernels -- vert_cell (offset to the type) holds GLOBAL cell slots, so those kernels index the whole tag array, tag_all,
// while a per-cell kernel indexes tag, which is offset to the type
struct TypeArrays : VertArrays { const int *vert_cell; int *tag_all; };

// ----------------------------------------------------------------------------
template <typename T>
inline int upload_vec(DevBuf<T> &dst, const std::vector<T> &src) {
  const int rc = dst.reserve(src.size() ? src.size() : 1); if (rc != HC_OK) return rc;
  if (src.size()) HC_HIP(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return HC_OK;
}
template <size_t N>
inline std::vector<int> flatten(const std::vector<std::array<long, N>> &v) {
  std::vector<int> o; o.reserve(v.size() * N);
  for (auto &a : v) for (long x : a) o.push_back((int)x);
  return o;
}

// storage management (cells.hip)
int sync_to_device(hc_cells *C);   // host staging -> device arrays when the host copy is newer
int sync_to_host(hc_cells *C);     // device arrays -> host staging before host-side edits
// make the host's view of the cell set current: reads the deletion counters (one small blocking copy, and only when an
// advance ran since the last time) and compacts gone cells away.  Every entry point that reports or edits cells calls it.
int settle(hc_cells *C);
TypeArrays vert_arrays(hc_cells *C, int t);
int ensure_sflag(hc_cells *C);     // solidify.hip: the flag array, zeroed, once a type is enabled and the vertex arrays exist
int solidify_refresh_mask(hc_cells *C);   // solidify.hip: hmask follows the device mask when nodes were solidified since (one host wait)
int solidify_check(hc_cells *C);   // solidify.hip: prepare, then flag, as hc_iterate runs them; no host wait
const char *solidify_refusal(const hc_lattice *L);   // solidify.hip: what on the lattice the feature does not combine with, or null
int ensure_rep(hc_cells *C);       // the three force_repulsion arrays, zeroed, once a repulsion is enabled and the vertex arrays exist
// stage a small host int array on the device in a persistent scratch slot (through a pinned block; stream ordered)
int stage_ints(hc_cells *C, int which, int **d, const int *h, int n);
int stage_ints(Staged<int> &s, int **d, const int *h, int n);   // the same through a staging block of the caller's
// the transposing copies between a staging [n][3] and three device arrays, from element `first` on (blocking)
int upload_xyz(DevBuf<double> dst[3], long first, const double *src, long n);
int download_xyz(double *dst, const DevBuf<double> src[3], long first, long n);
int append_cells(hc_cells *C, int type, const long *cell_ids, const int *is_new, int n, long n_new);   // exchange.hip: n_new cells join the end of a type's region (is_new null: all n)
int interpolate_cells_staged(hc_cells *C, int type, const int *slots, int n, int which);   // ibm.hip: hcp_interpolate_cells through staging slot `which`
inline int ibm_width(const hc_cells *C, int type) { return C->ibm_kernel[type]; }   // nodes per axis of the type's stencil

}  // namespace hcc
using namespace hcc;
