// Which lattice nodes lie inside a cell: the ray cast shared by the interior-viscosity pass (interior.hip) and the
// solidify pass (solidify.hip).
//
// Replaces (file:line in the HemoCell tree):
//   helper/octree.h:107-147    findInnerNodes: bounding box, parity of the ray crossings
//   helper/mollerTrumbore.h    the ray-triangle test
// Arithmetic follows mollerTrumbore.h and array.h operation for operation (-ffp-contract=off): every decision equals the
// numpy restatement in tests/interior_viscosity_ref.py bit for bit.
#pragma once
#include "cells.h"

namespace hcc {

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
// lattice_node() drops.  Args: anything with v (LatView), nv and px, py, pz offset to the type's first vertex.
template <class Args>
__device__ __forceinline__ void stage_cell(const Args &a, double *xs, double *ys, double *zs, int lo[3], int hi[3]) {
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

// number of triangles of the staged cell that the ray from the integer node (ox, oy, oz) crosses: the culls, then the exact test
__device__ __forceinline__ int ray_crossings(const double *xs, const double *ys, const double *zs, const int *tri, int nt, double ox, double oy, double oz) {
  const double oxy = ox - oy, oxz = ox - oz;
  int crossed = 0;
  for (int t = 0; t < nt; t++) {
    const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    const double v0x = xs[i0], v0y = ys[i0], v0z = zs[i0], v1x = xs[i1], v1y = ys[i1], v1z = zs[i1], v2x = xs[i2], v2y = ys[i2], v2z = zs[i2];
    if (min3(v0x, v1x, v2x) > ox + CULL_MARGIN || min3(v0y, v1y, v2y) > oy + CULL_MARGIN || min3(v0z, v1z, v2z) > oz + CULL_MARGIN) continue;
    const double d0 = v0x - v0y, d1 = v1x - v1y, d2 = v2x - v2y;
    if (min3(d0, d1, d2) > oxy + CULL_MARGIN || max3(d0, d1, d2) < oxy - CULL_MARGIN) continue;
    const double g0 = v0x - v0z, g1 = v1x - v1z, g2 = v2x - v2z;
    if (min3(g0, g1, g2) > oxz + CULL_MARGIN || max3(g0, g1, g2) < oxz - CULL_MARGIN) continue;
    crossed += moller_trumbore(v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z, ox, oy, oz);
  }
  return crossed;
}

}  // namespace hcc
