/*
 * hemo_oracle.c -- TEST INFRASTRUCTURE ONLY (see hemo_oracle.h).
 *
 * Plain-C fp64 restatement of the reference hot path.  Written in the
 * reference's own loop structure (scatter form, list order) so that summation
 * order follows the reference; compiled with -ffp-contract=off.
 */
#include "hemo_oracle.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define PI 3.14159265358979323846 /* config/constant_defaults.h:121-123 */

/* D3Q19, Palabos ordering (opposite of i is i+9, patch/palabos.patch:491-498) */
const int orc_c[ORC_Q][3] = {
    {0, 0, 0},  {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1},
    {-1, 0, 1}, {0, -1, -1}, {0, -1, 1}, {1, 0, 0},  {0, 1, 0},   {0, 0, 1},  {1, 1, 0},
    {1, -1, 0}, {1, 0, 1},  {1, 0, -1}, {0, 1, 1},  {0, 1, -1}};
const double orc_t[ORC_Q] = {1. / 3.,  1. / 18., 1. / 18., 1. / 18., 1. / 36., 1. / 36., 1. / 36.,
                             1. / 36., 1. / 36., 1. / 36., 1. / 18., 1. / 18., 1. / 18., 1. / 36.,
                             1. / 36., 1. / 36., 1. / 36., 1. / 36., 1. / 36.};

/* ======================================================================== */
/*                                 LATTICE                                  */
/* ======================================================================== */

orc_lattice *orc_lattice_create(int nx, int ny, int nz, const int periodic[3], double omega) {
  orc_lattice *L = (orc_lattice *)calloc(1, sizeof(orc_lattice));
  long n = (long)nx * ny * nz;
  L->nx = nx; L->ny = ny; L->nz = nz;
  for (int d = 0; d < 3; d++) L->periodic[d] = periodic[d];
  L->omega = omega;
  L->f = (double *)calloc((size_t)n * ORC_Q, sizeof(double));
  L->ftmp = (double *)calloc((size_t)n * ORC_Q, sizeof(double));
  L->force = (double *)calloc((size_t)n * 3, sizeof(double));
  L->mask = (unsigned char *)calloc((size_t)n, 1);
  L->nthreads = 1;
  return L;
}
void orc_lattice_destroy(orc_lattice *L) {
  if (!L) return;
  free(L->f); free(L->ftmp); free(L->force); free(L->mask); free(L->ob_code); free(L->ob_val); free(L);
}
void orc_lattice_set_threads(orc_lattice *L, int n) { L->nthreads = n < 1 ? 1 : n; }
void orc_lattice_set_wall_velocity(orc_lattice *L, int cls, const double u[3]) { for (int d = 0; d < 3; d++) L->wall_u[cls][d] = u[d]; }
void orc_lattice_set_mask(orc_lattice *L, const unsigned char *mask) {
  memcpy(L->mask, mask, (size_t)L->nx * L->ny * L->nz);
}

/* equilibrium in the fBar = f - t_i representation; Palabos
 * dynamicsTemplates::bgk_ma2_equilibrium: t_i*(rhoBar + 3 c.j + invRho*(4.5 (c.j)^2 - 1.5 j^2)) */
static double feq_bar(int i, double rhoBar, const double j[3], double jSqr) {
  double invRho = 1.0 / (1.0 + rhoBar);
  double c_j = orc_c[i][0] * j[0] + orc_c[i][1] * j[1] + orc_c[i][2] * j[2];
  return orc_t[i] * (rhoBar + 3.0 * c_j + invRho * (4.5 * c_j * c_j - 1.5 * jSqr));
}

/* core/hemoCell.cpp:129-133 latticeEquilibrium -> Palabos initializeAtEquilibrium.
 * BounceBack nodes: Palabos BounceBack::computeEquilibrium returns 0, i.e. fBar=0. */
void orc_lattice_init_equilibrium(orc_lattice *L, double rho, const double u[3]) {
  long n = (long)L->nx * L->ny * L->nz;
  double rhoBar = rho - 1.0;
  double j[3] = {rho * u[0], rho * u[1], rho * u[2]};
  double jSqr = j[0] * j[0] + j[1] * j[1] + j[2] * j[2];
#pragma omp parallel for num_threads(L->nthreads) schedule(static) if (L->nthreads > 1)
  for (long k = 0; k < n; k++)
    for (int i = 0; i < ORC_Q; i++) L->f[k * ORC_Q + i] = L->mask[k] ? 0.0 : feq_bar(i, rhoBar, j, jSqr);
}

/* setExternalVector(lattice, bbox, forceBeginsAt, F) (core/hemoCell.cpp:369-371,
 * examples/pipeflow/pipeflow.cpp:144-146) */
void orc_lattice_set_force_uniform(orc_lattice *L, const double F[3]) {
  long n = (long)L->nx * L->ny * L->nz;
#pragma omp parallel for num_threads(L->nthreads) schedule(static) if (L->nthreads > 1)
  for (long k = 0; k < n; k++) { L->force[3 * k] = F[0]; L->force[3 * k + 1] = F[1]; L->force[3 * k + 2] = F[2]; }
}

/* the same call with a sub-domain (cases/kolmogorovFlow/kolmogorovFlow.cpp:136-140); box = inclusive {x0,x1,y0,y1,z0,z1} */
void orc_lattice_set_force_box(orc_lattice *L, const int box[6], const double F[3]) {
  for (int x = box[0] < 0 ? 0 : box[0]; x <= box[1] && x < L->nx; x++)
    for (int y = box[2] < 0 ? 0 : box[2]; y <= box[3] && y < L->ny; y++)
      for (int z = box[4] < 0 ? 0 : box[4]; z <= box[5] && z < L->nz; z++) {
        long k = ((long)x * L->ny + y) * L->nz + z;
        L->force[3 * k] = F[0]; L->force[3 * k + 1] = F[1]; L->force[3 * k + 2] = F[2];
      }
}

static inline void moments(const double *f, double *rhoBar, double j[3]) {
  double r = 0, jx = 0, jy = 0, jz = 0;
  for (int i = 0; i < ORC_Q; i++) {
    r += f[i];
    jx += orc_c[i][0] * f[i];
    jy += orc_c[i][1] * f[i];
    jz += orc_c[i][2] * f[i];
  }
  *rhoBar = r; j[0] = jx; j[1] = jy; j[2] = jz;
}

void orc_lattice_set_open_boundary(orc_lattice *L, const int *code, const double *val) {
  const long n = (long)L->nx * L->ny * L->nz;
  free(L->ob_code); free(L->ob_val); L->ob_code = NULL; L->ob_val = NULL;
  if (!code) return;
  long slots = 0;
  for (long k = 0; k < n; k++) if (code[k] >= 0 && (code[k] >> 2) + 1 > slots) slots = (code[k] >> 2) + 1;
  L->ob_code = (int *)malloc((size_t)n * sizeof(int));
  memcpy(L->ob_code, code, (size_t)n * sizeof(int));
  L->ob_val = (double *)malloc((size_t)(slots ? slots : 1) * 4 * sizeof(double));
  if (slots) memcpy(L->ob_val, val, (size_t)slots * 4 * sizeof(double));
}

/* Zou-He completion with normal x on stored-form populations (f_i - t_i; the opposite populations of a pair share t_i, and
 * the t_i of the nine c_x = 0 and twice the five outgoing populations add up to 1).  0N (kind even): the five populations
 * with c_x = +1 are unknown,
 *   rho = (S_0 + 2 S_-) / (1 - u_x)   [pressure nodes: rho given, u_x = 1 - (S_0 + 2 S_-) / rho, u_y = u_z = 0]
 *   f(1,0,0) = f(-1,0,0) + rho u_x / 3,  f(1,+-1,0) = f(-1,-+1,0) + rho (u_x +- u_y) / 6 -+ N_y,  likewise z,
 *   N_y = (sum over c = (0,1,.) - sum over c = (0,-1,.)) / 2 - rho u_y / 3;
 * 0P mirrors it with rho = (S_0 + 2 S_+) / (1 + u_x).  Palabos is not in the tree: the operation order is this project's. */
static void zou_he_x(double *f, int code, const double *val) {
  const int kind = code & 3, neg = (kind & 1) == 0;
  const double *v = val + 4 * (long)(code >> 2);
  const double s0 = f[0] + f[2] + f[3] + f[8] + f[9] + f[11] + f[12] + f[17] + f[18];
  const double sm = f[1] + f[4] + f[5] + f[6] + f[7];
  const double sp = f[10] + f[13] + f[14] + f[15] + f[16];
  const double known = s0 + 2.0 * (neg ? sm : sp) + 1.0;
  double rho, ux, uy, uz;
  if (kind < 2) {
    ux = v[0]; uy = v[1]; uz = v[2];
    rho = neg ? known / (1.0 - ux) : known / (1.0 + ux);
  } else {
    rho = v[3];
    ux = neg ? 1.0 - known / rho : known / rho - 1.0;
    uy = 0.0; uz = 0.0;
  }
  const double ny = 0.5 * ((f[11] + f[17] + f[18]) - (f[2] + f[8] + f[9])) - rho * uy / 3.0;
  const double nz = 0.5 * ((f[12] + f[9] + f[17]) - (f[3] + f[8] + f[18])) - rho * uz / 3.0;
  if (neg) {
    f[10] = f[1] + rho * ux / 3.0;
    f[13] = f[4] + rho * (ux + uy) / 6.0 - ny;
    f[14] = f[5] + rho * (ux - uy) / 6.0 + ny;
    f[15] = f[6] + rho * (ux + uz) / 6.0 - nz;
    f[16] = f[7] + rho * (ux - uz) / 6.0 + nz;
  } else {
    f[1] = f[10] - rho * ux / 3.0;
    f[4] = f[13] - rho * (ux + uy) / 6.0 + ny;
    f[5] = f[14] - rho * (ux - uy) / 6.0 - ny;
    f[6] = f[15] - rho * (ux + uz) / 6.0 + nz;
    f[7] = f[16] - rho * (ux - uz) / 6.0 - nz;
  }
}
static inline int open_code(const orc_lattice *L, long k) { return (L->ob_code && !L->mask[k]) ? L->ob_code[k] : -1; }

/* Cell::computeVelocity for ExternalForceDynamics: u = j*invRho + F/2 (SURVEY A6;
 * used by core/hemoCellParticleField.cpp:833) */
void orc_node_rho_u(const orc_lattice *L, long node, double *rho, double u[3]) {
  double rhoBar, j[3];
  const int code = open_code(L, node);
  if (code >= 0) {   /* an open-boundary node reports the moments of the completed populations: what its collide relaxes */
    double g[ORC_Q];
    for (int i = 0; i < ORC_Q; i++) g[i] = L->f[node * ORC_Q + i];
    zou_he_x(g, code, L->ob_val);
    moments(g, &rhoBar, j);
  } else moments(L->f + node * ORC_Q, &rhoBar, j);
  double invRho = 1.0 / (1.0 + rhoBar);
  *rho = 1.0 + rhoBar;
  for (int d = 0; d < 3; d++) u[d] = j[d] * invRho + L->force[3 * node + d] / 2.0;
}

/* GuoExternalForceBGKdynamics::collide (Palabos; restated):
 *   rhoBar, u = j/rho + F/2 ; j := rho*u ; BGK relax to 2nd order equilibrium ;
 *   f_i += (1-omega/2) t_i [ (c_i-u)*3 + 9 (c_i.u) c_i ] . F                    */
static void collide_guo_bgk(double *f, const double *F, double omega) {
  double rhoBar, j[3], u[3];
  moments(f, &rhoBar, j);
  double invRho = 1.0 / (1.0 + rhoBar);
  double rho = 1.0 + rhoBar;
  for (int d = 0; d < 3; d++) { u[d] = j[d] * invRho + F[d] / 2.0; j[d] = rho * u[d]; }
  double jSqr = j[0] * j[0] + j[1] * j[1] + j[2] * j[2];
  for (int i = 0; i < ORC_Q; i++) {
    f[i] *= (1.0 - omega);
    f[i] += omega * feq_bar(i, rhoBar, j, jSqr);
  }
  for (int i = 0; i < ORC_Q; i++) {
    double c_u = orc_c[i][0] * u[0] + orc_c[i][1] * u[1] + orc_c[i][2] * u[2];
    c_u *= 9.0; /* invCs2*invCs2 */
    double forceTerm = 0.0;
    for (int d = 0; d < 3; d++) forceTerm += (((double)orc_c[i][d] - u[d]) * 3.0 + c_u * (double)orc_c[i][d]) * F[d];
    forceTerm *= orc_t[i];
    forceTerm *= 1.0 - omega / 2.0;
    f[i] += forceTerm;
  }
}

/* BounceBack::collide: swap f[i] <-> f[i+9], i=1..9 */
static void collide_bounce_back(double *f) {
  for (int i = 1; i <= 9; i++) { double t = f[i]; f[i] = f[i + 9]; f[i + 9] = t; }
}
/* Moving no-slip wall (mask classes 3..6): full-way bounce-back with Ladd's momentum term at rho = 1,
 * f_opp(i) = f_i - 2 t_i (c_i.u_w)/cs^2.  This is the stand-in for Palabos' regularised velocity boundary
 * (createLocalBoundaryCondition3D, examples/oneCellShear/oneCellShear.cpp:62-66), which is not available;
 * the two agree on the flow they impose, not bit for bit (UNPINNED). */
static void collide_moving_wall(double *f, const double *uw) {
  double in[ORC_Q];
  for (int i = 0; i < ORC_Q; i++) in[i] = f[i];
  for (int i = 1; i < ORC_Q; i++) {
    const int o = i <= 9 ? i + 9 : i - 9;
    const double c_u = orc_c[i][0] * uw[0] + orc_c[i][1] * uw[1] + orc_c[i][2] * uw[2];
    f[o] = in[i] - 6.0 * orc_t[i] * c_u;
  }
}

/* MultiBlockLattice3D::collideAndStream (core/hemoCell.cpp:317): collide every
 * node, then stream f_i(x+c_i) <- f*_i(x) with periodic wrap
 * (patch/palabos.patch:459-466 implements it as in-place swaps; the net effect
 * is the plain collide -> stream done here with two buffers).  A population
 * whose source lies outside a non-periodic face is set to fBar = 0 (only
 * wall/BC nodes sit on such faces in the in-scope cases, so the value never
 * reaches a fluid node). */
void orc_collide_stream(orc_lattice *L) {
  const int nx = L->nx, ny = L->ny, nz = L->nz;
  const long n = (long)nx * ny * nz;
  if (L->fused) { orc_collide_stream_fused(L); return; }
  memcpy(L->ftmp, L->f, (size_t)n * ORC_Q * sizeof(double));
#ifdef _OPENMP
#pragma omp parallel for num_threads(L->nthreads) schedule(static)
#endif
  for (long k = 0; k < n; k++) {
    if (L->mask[k] >= 3) collide_moving_wall(L->ftmp + k * ORC_Q, L->wall_u[L->mask[k] - 3]);
    else if (L->mask[k]) collide_bounce_back(L->ftmp + k * ORC_Q);
    else {
      const int code = open_code(L, k);
      if (code >= 0) zou_he_x(L->ftmp + k * ORC_Q, code, L->ob_val);
      collide_guo_bgk(L->ftmp + k * ORC_Q, L->force + 3 * k, L->omega);
    }
  }
#ifdef _OPENMP
#pragma omp parallel for num_threads(L->nthreads) schedule(static)
#endif
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
      for (int z = 0; z < nz; z++) {
        long k = z + (long)nz * (y + (long)ny * x);
        for (int i = 0; i < ORC_Q; i++) {
          int sx = x - orc_c[i][0], sy = y - orc_c[i][1], sz = z - orc_c[i][2];
          int ok = 1;
          if (sx < 0 || sx >= nx) { if (L->periodic[0]) sx = (sx + nx) % nx; else ok = 0; }
          if (sy < 0 || sy >= ny) { if (L->periodic[1]) sy = (sy + ny) % ny; else ok = 0; }
          if (sz < 0 || sz >= nz) { if (L->periodic[2]) sz = (sz + nz) % nz; else ok = 0; }
          L->f[k * ORC_Q + i] = ok ? L->ftmp[(sz + (long)nz * (sy + (long)ny * sx)) * ORC_Q + i] : 0.0;
        }
      }
}

/* The same step in one pass: every node is collided in a local copy and its 19 post-collision values are pushed to
 * the neighbours' slots of the second buffer (f_i(x+c_i) <- f*_i(x)); the buffers are then swapped.  Slots whose source
 * lies outside a non-periodic face are set to 0 first, as above.  The operations on every value are those of
 * orc_collide_stream in the same order, so the result is bit-identical (tests/test_oracle_pins.py); only the data
 * movement differs (one read and one write of the populations instead of three of each). */
void orc_collide_stream_fused(orc_lattice *L) {
  const int nx = L->nx, ny = L->ny, nz = L->nz;
  double *restrict src = L->f, *restrict dst = L->ftmp;
  /* faces without a source (non-periodic axes): fBar = 0 for the populations that would come from outside */
  for (int d = 0; d < 3; d++) {
    if (L->periodic[d]) continue;
    const int nd = d == 0 ? nx : d == 1 ? ny : nz;
    for (int side = 0; side < 2; side++) {
      const int at = side ? nd - 1 : 0;
      if (nd == 1 && side) continue;
      const int na = d == 0 ? ny : nx, nb = d == 2 ? ny : nz;
#ifdef _OPENMP
#pragma omp parallel for num_threads(L->nthreads) schedule(static) if (L->nthreads > 1)
#endif
      for (int a = 0; a < na; a++)
        for (int b = 0; b < nb; b++) {
          const int x = d == 0 ? at : a, y = d == 1 ? at : (d == 0 ? a : b), z = d == 2 ? at : b;
          const long k = z + (long)nz * (y + (long)ny * x);
          for (int i = 0; i < ORC_Q; i++) {
            const int s = at - orc_c[i][d];
            if (s < 0 || s >= nd) dst[k * ORC_Q + i] = 0.0;
          }
        }
    }
  }
#ifdef _OPENMP
#pragma omp parallel for num_threads(L->nthreads) schedule(static)
#endif
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++)
      for (int z = 0; z < nz; z++) {
        const long k = z + (long)nz * (y + (long)ny * x);
        double f[ORC_Q];
        for (int i = 0; i < ORC_Q; i++) f[i] = src[k * ORC_Q + i];
        if (L->mask[k] >= 3) collide_moving_wall(f, L->wall_u[L->mask[k] - 3]);
        else if (L->mask[k]) collide_bounce_back(f);
        else {
          const int code = open_code(L, k);
          if (code >= 0) zou_he_x(f, code, L->ob_val);
          collide_guo_bgk(f, L->force + 3 * k, L->omega);
        }
        for (int i = 0; i < ORC_Q; i++) {
          int tx = x + orc_c[i][0], ty = y + orc_c[i][1], tz = z + orc_c[i][2];
          if (tx < 0 || tx >= nx) { if (L->periodic[0]) tx = (tx + nx) % nx; else continue; }
          if (ty < 0 || ty >= ny) { if (L->periodic[1]) ty = (ty + ny) % ny; else continue; }
          if (tz < 0 || tz >= nz) { if (L->periodic[2]) tz = (tz + nz) % nz; else continue; }
          dst[(tz + (long)nz * (ty + (long)ny * tx)) * ORC_Q + i] = f[i];
        }
      }
  L->f = dst; L->ftmp = src;
}

/* ======================================================================== */
/*                               PARAMETERS                                 */
/* ======================================================================== */

/* Parameters::lbm_base_parameters, mechanics/constantConversion.cpp:36-59 */
void orc_params_base(orc_params *P, double dx, double dt, double nu_p, double rho_p, double kBT_p) {
  P->dx = dx; P->dt = dt; P->nu_p = nu_p; P->rho_p = rho_p; P->kBT_p = kBT_p;
  if (dt < 0.0) {
    P->tau = 1.0;
    P->nu_lbm = 1.0 / 3.0 * (P->tau - 0.5);
    P->dt = P->nu_lbm / nu_p * (dx * dx);
  } else {
    P->nu_lbm = nu_p * dt / (dx * dx);
    P->tau = 3.0 * P->nu_lbm + 0.5;
  }
  P->dm = rho_p * (dx * dx * dx);
  P->df = P->dm * dx / (P->dt * P->dt);
  P->f_limit = 50.0 / 1.0e12 / P->df; /* FORCE_LIMIT 50 pN, config/constant_defaults.h:73-75 */
  P->kBT_lbm = kBT_p / (P->df * dx);
}

/* ======================================================================== */
/*                         SMALL VECTOR HELPERS                             */
/* ======================================================================== */
static inline void v_sub(const double *a, const double *b, double *r) { r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; }
static inline void v_cross(const double *a, const double *b, double *r) {
  r[0] = a[1] * b[2] - a[2] * b[1];
  r[1] = a[2] * b[0] - a[0] * b[2];
  r[2] = a[0] * b[1] - a[1] * b[0];
}
/* helper/array.h:228-244: accumulating loops starting from 0 */
static inline double v_dot(const double *a, const double *b) { double r = 0; for (int i = 0; i < 3; i++) r += a[i] * b[i]; return r; }
static inline double v_norm(const double *a) { double r = 0; for (int i = 0; i < 3; i++) r += a[i] * a[i]; return sqrt(r); }

/* helper/array.h:270-285 computeTriangleAreaAndUnitNormal */
static void tri_area_unit_normal(const double *v0, const double *v1, const double *v2, double *area, double *n) {
  double e01[3], e02[3];
  v_sub(v1, v0, e01); v_sub(v2, v0, e02);
  v_cross(e01, e02, n);
  double normN = v_norm(n);
  if (normN != 0.0) { *area = 0.5 * normN; n[0] /= normN; n[1] /= normN; n[2] /= normN; }
  else { *area = 0; n[0] = n[1] = n[2] = 0; }
}
/* helper/array.h:287-304 computeTriangleNormal(..., isAreaWeighted=false) */
static void tri_unit_normal(const double *v0, const double *v1, const double *v2, double *n) {
  double e01[3], e02[3];
  v_sub(v1, v0, e01); v_sub(v2, v0, e02);
  v_cross(e01, e02, n);
  double normN = v_norm(n);
  if (normN != 0) { n[0] /= normN; n[1] /= normN; n[2] /= normN; } else { n[0] = n[1] = n[2] = 0; }
}
/* helper/geometryUtils.h:49-52 */
static double angle_between_faces(const double *n1, const double *n2, const double *edge) {
  double cr[3]; v_cross(n1, n2, cr);
  return atan2(v_dot(cr, edge), v_dot(n1, n2));
}

/* ======================================================================== */
/*                        MESH GENERATION (setup, a10)                      */
/* ======================================================================== */
typedef struct { double v[3][3]; } tri3;

/* Palabos TriangleSet<T>::rotate(phi,theta,psi): z-x-z Euler, R = Rz(psi) Rx(theta) Rz(phi)
 * (restated; Palabos is not in the reference tree) */
static void triset_rotate(tri3 *t, long nt, double phi, double theta, double psi) {
  double a[3][3] = {{1, 0, 0}, {0, cos(theta), -sin(theta)}, {0, sin(theta), cos(theta)}};
  double b[3][3] = {{cos(phi), -sin(phi), 0}, {sin(phi), cos(phi), 0}, {0, 0, 1}};
  double c[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { c[i][j] = 0; for (int k = 0; k < 3; k++) c[i][j] += a[i][k] * b[k][j]; }
  double b2[3][3] = {{cos(psi), -sin(psi), 0}, {sin(psi), cos(psi), 0}, {0, 0, 1}};
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { a[i][j] = 0; for (int k = 0; k < 3; k++) a[i][j] += b2[i][k] * c[k][j]; }
  for (long it = 0; it < nt; it++) for (int iv = 0; iv < 3; iv++) {
    double x[3] = {t[it].v[iv][0], t[it].v[iv][1], t[it].v[iv][2]};
    for (int i = 0; i < 3; i++) { double s = 0; for (int j = 0; j < 3; j++) s += a[i][j] * x[j]; t[it].v[iv][i] = s; }
  }
}

static void refine_sphere(tri3 **pt, long *pnt, long minTri) {
  /* helper/meshGeneratingFunctions.hh:109-146: split each triangle in 4,
   * midpoints pushed to the unit sphere; triangle i is REPLACED by the centre
   * triangle and the three corner triangles are appended */
  tri3 *t = *pt; long size;
  while ((size = *pnt) < minTri) {
    t = (tri3 *)realloc(t, sizeof(tri3) * (size_t)size * 4);
    long cnt = size;
    for (long i = 0; i < size; i++) {
      double va[3], vb[3], vc[3], vd[3], ve[3], vf[3];
      memcpy(va, t[i].v[0], 24); memcpy(vb, t[i].v[1], 24); memcpy(vc, t[i].v[2], 24);
      for (int d = 0; d < 3; d++) { vd[d] = 0.5 * (va[d] + vb[d]); ve[d] = 0.5 * (vb[d] + vc[d]); vf[d] = 0.5 * (vc[d] + va[d]); }
      double nd = v_norm(vd), ne = v_norm(ve), nf = v_norm(vf);
      for (int d = 0; d < 3; d++) { vd[d] /= nd; ve[d] /= ne; vf[d] /= nf; }
      memcpy(t[i].v[0], vd, 24); memcpy(t[i].v[1], ve, 24); memcpy(t[i].v[2], vf, 24);
      memcpy(t[cnt].v[0], va, 24); memcpy(t[cnt].v[1], vd, 24); memcpy(t[cnt].v[2], vf, 24); cnt++;
      memcpy(t[cnt].v[0], vd, 24); memcpy(t[cnt].v[1], vb, 24); memcpy(t[cnt].v[2], ve, 24); cnt++;
      memcpy(t[cnt].v[0], vf, 24); memcpy(t[cnt].v[1], ve, 24); memcpy(t[cnt].v[2], vc, 24); cnt++;
    }
    *pnt = cnt;
  }
  *pt = t;
}

/* helper/meshGeneratingFunctions.hh:32-153 constructSphereIcosahedron (unit sphere) */
static tri3 *sphere_icosahedron(long minTri, long *pnt) {
  const double tau = -0.8506508084, one = -0.5257311121;
  const double V[12][3] = {{tau, one, 0}, {-tau, one, 0}, {-tau, -one, 0}, {tau, -one, 0},
                           {one, 0, tau}, {one, 0, -tau}, {-one, 0, -tau}, {-one, 0, tau},
                           {0, tau, one}, {0, -tau, one}, {0, -tau, -one}, {0, tau, -one}};
  /* 1-based v1..v12 as in the reference */
  static const int F[20][3] = {{5, 8, 9}, {5, 10, 8}, {6, 12, 7}, {6, 7, 11}, {1, 4, 5}, {1, 6, 4}, {3, 2, 8},
                               {3, 7, 2}, {9, 12, 1}, {9, 2, 12}, {10, 4, 11}, {10, 11, 3}, {9, 1, 5},
                               {12, 6, 1}, {5, 4, 10}, {6, 11, 4}, {8, 2, 9}, {7, 12, 2}, {8, 10, 3}, {7, 3, 11}};
  tri3 *t = (tri3 *)malloc(sizeof(tri3) * 20);
  for (int i = 0; i < 20; i++) for (int k = 0; k < 3; k++) memcpy(t[i].v[k], V[F[i][k] - 1], 24);
  *pnt = 20;
  refine_sphere(&t, pnt, minTri);
  return t;
}

/* Palabos constructSphere (octahedron start; helper/meshGeneratingFunctions.h:55
 * "initialSphereShape [0] Octahedron (PLB Sphere)"); restated from the Palabos
 * generator the icosahedron routine above was derived from -- UNPINNED. */
static tri3 *sphere_octahedron(long minTri, long *pnt) {
  const double va[3] = {1, 0, 0}, vb[3] = {0, 1, 0}, vc[3] = {-1, 0, 0}, vd[3] = {0, -1, 0}, ve[3] = {0, 0, 1}, vf[3] = {0, 0, -1};
  const double *F[8][3] = {{ve, va, vb}, {ve, vb, vc}, {ve, vc, vd}, {ve, vd, va}, {vf, vb, va}, {vf, vc, vb}, {vf, vd, vc}, {vf, va, vd}};
  tri3 *t = (tri3 *)malloc(sizeof(tri3) * 8);
  for (int i = 0; i < 8; i++) for (int k = 0; k < 3; k++) memcpy(t[i].v[k], F[i][k], 24);
  *pnt = 8;
  refine_sphere(&t, pnt, minTri);
  return t;
}

/* helper/meshGeneratingFunctions.hh:155-171 spherePointToRBCPoint (R = 1) */
static void sphere_to_rbc(double *p) {
  double r2 = p[0] * p[0] + p[1] * p[1];
  double val = p[2];
  int sign = (0.0 < val) - (val < 0.0);
  if (1 - r2 < 0) r2 = 1;
  const double C0 = 0.054322, C2 = 1.001279, C4 = -0.561381;
  p[2] = sign * 1.0 * sqrt(1 - r2) * (C0 + C2 * r2 + C4 * r2 * r2);
}
/* helper/meshGeneratingFunctions.hh:173-186 spherePointToEllipsoidPoint */
static void sphere_to_ellipsoid(double *p, double R, double aspect) {
  double r2 = p[0] * p[0] + p[1] * p[1];
  double val = p[2];
  int sign = (0.0 < val) - (val < 0.0);
  if (1 - r2 < 0) r2 = 1;
  p[0] *= R; p[1] *= R;
  p[2] = sign * aspect * R * sqrt(1 - r2);
}

/* constructRBCFromSphere / constructEllipsoidFromSphere
 * (helper/meshGeneratingFunctions.hh:217-271), eulerAngles = 0, centre = 0 */
static tri3 *make_shape(int shape, double radius, long minTri, double aspect, long *pnt) {
  tri3 *t;
  if (shape == 1) {
    t = sphere_icosahedron(minTri, pnt);
    triset_rotate(t, *pnt, PI / 2.0, PI / 2.0, 0.);
    for (long i = 0; i < *pnt; i++) for (int k = 0; k < 3; k++) sphere_to_rbc(t[i].v[k]);
    for (long i = 0; i < *pnt; i++) for (int k = 0; k < 3; k++) for (int d = 0; d < 3; d++) t[i].v[k][d] *= radius;
    triset_rotate(t, *pnt, PI / 2.0, PI / 2.0, 0.);
  } else {
    t = sphere_octahedron(minTri, pnt);
    triset_rotate(t, *pnt, PI / 2.0, PI / 2.0, 0.);
    for (long i = 0; i < *pnt; i++) for (int k = 0; k < 3; k++) sphere_to_ellipsoid(t[i].v[k], radius, aspect);
    triset_rotate(t, *pnt, PI / 2.0, PI / 2.0, 0.);
  }
  return t;
}

/* TriangleSet -> DEFscaledMesh -> TriangleBoundary3D (helper/meshGeneratingFunctions.h:89-92):
 * vertices numbered in first-occurrence order over the triangle list (Palabos
 * TriangleToDef; UNPINNED -- see SURVEY "Hard parts").  mesh.inflate() moves
 * vertices by a negligible epsilon and is omitted. */
static void dedupe(const tri3 *t, long nt, double **pv, long *pnv, long **ptri) {
  double *v = (double *)malloc(sizeof(double) * 3 * (size_t)nt * 3);
  long *tri = (long *)malloc(sizeof(long) * 3 * (size_t)nt);
  long nv = 0;
  const double eps = 1e-9;
  for (long i = 0; i < nt; i++) for (int k = 0; k < 3; k++) {
    const double *p = t[i].v[k];
    long found = -1;
    for (long q = 0; q < nv; q++)
      if (fabs(v[3 * q] - p[0]) < eps && fabs(v[3 * q + 1] - p[1]) < eps && fabs(v[3 * q + 2] - p[2]) < eps) { found = q; break; }
    if (found < 0) { memcpy(v + 3 * nv, p, 24); found = nv++; }
    tri[3 * i + k] = found;
  }
  *pv = v; *pnv = nv; *ptri = tri;
}

/* Cells.getMesh().inflate() (helper/meshGeneratingFunctions.h:92): Palabos
 * TriangularSurfaceMesh::inflate moves every vertex along its vertex normal
 * (normalised sum of the incident triangles' unit normals) by a small amount.
 * Palabos is absent, so the amount is UNPINNED; 1e-3 lattice units is the value
 * for which the undeformed RBC volume (81.116 um^3) is consistent with the
 * 81.12-81.19 um^3 / 100-100.1 % band of scripts/ci/stretchCell_sanity.sh:19-26
 * (without inflation the mesh volume is 81.052 um^3, outside that band). */
static void mesh_inflate(orc_celltype *T, double amount) {
  double *vn = (double *)calloc((size_t)T->nv * 3, sizeof(double));
  for (long t = 0; t < T->nt; t++) {
    const long *tr = T->triangles + 3 * t; double n[3];
    tri_unit_normal(T->vertices + 3 * tr[0], T->vertices + 3 * tr[1], T->vertices + 3 * tr[2], n);
    for (int k = 0; k < 3; k++) for (int d = 0; d < 3; d++) vn[3 * tr[k] + d] += n[d];
  }
  for (long i = 0; i < T->nv; i++) {
    double l = v_norm(vn + 3 * i);
    for (int d = 0; d < 3; d++) T->vertices[3 * i + d] += amount * (vn[3 * i + d] / l);
  }
  free(vn);
}

/* Palabos TriangularSurfaceMesh::getAdjacentTriangleIds(i,j) (absent).  For a
 * closed oriented manifold exactly one triangle holds the directed edge i->j and
 * one holds j->i.  Order returned here: [0] = triangle with directed edge j->i,
 * [1] = triangle with i->j.  With outward-wound triangles this is the order for
 * which pltSimpleModel's dihedral bending force is restoring (UNPINNED). */
static void adjacent_triangles(const orc_celltype *T, long i, long j, long out[2]) {
  out[0] = out[1] = -1;
  for (long t = 0; t < T->nt; t++) {
    const long *tr = T->triangles + 3 * t;
    for (int k = 0; k < 3; k++) {
      if (tr[k] == i && tr[(k + 1) % 3] == j) out[1] = t;
      if (tr[k] == j && tr[(k + 1) % 3] == i) out[0] = t;
    }
  }
}

/* CommonCellConstants::CommonCellConstantsConstructor, mechanics/commonCellConstants.cpp:70-409 */
static void build_tables(orc_celltype *T, const long *inner, int n_inner) {
  const long nv = T->nv, nt = T->nt;
  /* edges: mechanics/commonCellConstants.cpp:81-93 */
  T->edges = (long *)malloc(sizeof(long) * 2 * 3 * (size_t)nt);
  long ne = 0;
  for (long t = 0; t < nt; t++) {
    const long *tr = T->triangles + 3 * t;
    if (tr[0] < tr[1]) { T->edges[2 * ne] = tr[0]; T->edges[2 * ne + 1] = tr[1]; ne++; }
    if (tr[1] < tr[2]) { T->edges[2 * ne] = tr[1]; T->edges[2 * ne + 1] = tr[2]; ne++; }
    if (tr[2] < tr[0]) { T->edges[2 * ne] = tr[2]; T->edges[2 * ne + 1] = tr[0]; ne++; }
  }
  T->ne = (int)ne;
  T->edge_length_eq = (double *)malloc(sizeof(double) * (size_t)ne);
  T->edge_angle_eq = (double *)malloc(sizeof(double) * (size_t)ne);
  T->edge_bending_triangles = (long *)malloc(sizeof(long) * 2 * (size_t)ne);
  T->edge_bending_outer = (long *)malloc(sizeof(long) * 2 * (size_t)ne);
  for (long e = 0; e < ne; e++) {
    const double *p0 = T->vertices + 3 * T->edges[2 * e], *p1 = T->vertices + 3 * T->edges[2 * e + 1];
    double d[3]; v_sub(p1, p0, d); /* :96-99 computeEdgeLength */
    T->edge_length_eq[e] = v_norm(d);
  }
  for (long e = 0; e < ne; e++) { /* :101-137 and :162-179 */
    long e0 = T->edges[2 * e], e1 = T->edges[2 * e + 1], adj[2];
    adjacent_triangles(T, e0, e1, adj);
    const long *ta = T->triangles + 3 * adj[0], *tb = T->triangles + 3 * adj[1];
    double V1[3], V2[3];
    tri_unit_normal(T->vertices + 3 * ta[0], T->vertices + 3 * ta[1], T->vertices + 3 * ta[2], V1);
    tri_unit_normal(T->vertices + 3 * tb[0], T->vertices + 3 * tb[1], T->vertices + 3 * tb[2], V2);
    double ev[3]; v_sub(T->vertices + 3 * e1, T->vertices + 3 * e0, ev);
    double el = v_norm(ev); ev[0] /= el; ev[1] /= el; ev[2] /= el;
    T->edge_angle_eq[e] = angle_between_faces(V1, V2, ev);
    T->edge_bending_triangles[2 * e] = adj[0]; T->edge_bending_triangles[2 * e + 1] = adj[1];
    for (int i = 0; i < 3; i++) {
      if (ta[i] != e0 && ta[i] != e1) T->edge_bending_outer[2 * e] = ta[i];
      if (tb[i] != e0 && tb[i] != e1) T->edge_bending_outer[2 * e + 1] = tb[i];
    }
  }
  /* inner edges :139-159 */
  T->nie = n_inner;
  T->inner_edges = (long *)malloc(sizeof(long) * 2 * (size_t)(n_inner > 0 ? n_inner : 1));
  T->inner_edge_length_eq = (double *)malloc(sizeof(double) * (size_t)(n_inner > 0 ? n_inner : 1));
  for (int e = 0; e < n_inner; e++) {
    T->inner_edges[2 * e] = inner[2 * e]; T->inner_edges[2 * e + 1] = inner[2 * e + 1];
    double d[3]; v_sub(T->vertices + 3 * inner[2 * e + 1], T->vertices + 3 * inner[2 * e], d);
    T->inner_edge_length_eq[e] = v_norm(d);
  }
  /* triangle areas :155-159 */
  T->triangle_area_eq = (double *)malloc(sizeof(double) * (size_t)nt);
  for (long t = 0; t < nt; t++) {
    const long *tr = T->triangles + 3 * t; double a, n[3];
    tri_area_unit_normal(T->vertices + 3 * tr[0], T->vertices + 3 * tr[1], T->vertices + 3 * tr[2], &a, n);
    T->triangle_area_eq[t] = a;
  }
  /* volume_eq: MeshMetrics::getVolume, helper/meshMetrics.h:167-177 (every
   * triangle visited once per corner, /6/3 each time) */
  double vol = 0.0;
  for (long iv = 0; iv < nv; iv++)
    for (long t = 0; t < nt; t++) {
      const long *tr = T->triangles + 3 * t;
      if (tr[0] != iv && tr[1] != iv && tr[2] != iv) continue;
      double tmp[3]; v_cross(T->vertices + 3 * tr[1], T->vertices + 3 * tr[2], tmp);
      vol += v_dot(T->vertices + 3 * tr[0], tmp) / 6.0 / 3.0;
    }
  T->volume_eq = vol;
  /* means :181-199 */
  double s = 0; for (long t = 0; t < nt; t++) s += T->triangle_area_eq[t]; T->area_mean_eq = s / nt;
  s = 0; for (long e = 0; e < ne; e++) s += T->edge_length_eq[e]; T->edge_mean_eq = s / ne;
  s = 0; for (long e = 0; e < ne; e++) s += T->edge_angle_eq[e]; T->angle_mean_eq = s / ne;
  /* vertex neighbours :201-228 */
  T->vertex_vertexes = (long *)malloc(sizeof(long) * 6 * (size_t)nv);
  T->vertex_n_vertexes = (int *)calloc((size_t)nv, sizeof(int));
  for (long i = 0; i < 6 * nv; i++) T->vertex_vertexes[i] = -1;
  for (long e = 0; e < ne; e++) {
    long a = T->edges[2 * e], b = T->edges[2 * e + 1];
    for (int k = 0; k < 6; k++) if (T->vertex_vertexes[6 * a + k] == -1) { T->vertex_vertexes[6 * a + k] = b; break; }
    for (int k = 0; k < 6; k++) if (T->vertex_vertexes[6 * b + k] == -1) { T->vertex_vertexes[6 * b + k] = a; break; }
  }
  for (long i = 0; i < nv; i++) for (int k = 0; k < 6; k++) if (T->vertex_vertexes[6 * i + k] != -1) T->vertex_n_vertexes[i]++;
  /* ring ordering :231-271: next = third vertex of the triangle that holds the
   * directed edge (vertex -> n_vertex) */
  for (long v = 0; v < nv; v++) {
    long n_vertex = T->vertex_vertexes[6 * v], next = -1;
    for (int n = 1; n < T->vertex_n_vertexes[v]; n++) {
      for (long t = 0; t < nt; t++) {
        const long *tr = T->triangles + 3 * t;
        for (int k = 0; k < 3; k++)
          if (tr[k] == v && tr[(k + 1) % 3] == n_vertex) next = tr[(k + 2) % 3];
      }
      n_vertex = next;
      T->vertex_vertexes[6 * v + n] = n_vertex;
    }
  }
  /* patch centre distance :274-305 */
  T->patch_dist_eq = (double *)malloc(sizeof(double) * (size_t)nv);
  for (long i = 0; i < nv; i++) {
    int nn = T->vertex_n_vertexes[i];
    const long *ring = T->vertex_vertexes + 6 * i;
    const double *x = T->vertices + 3 * i;
    double sum[3] = {0, 0, 0};
    for (int j = 0; j < nn; j++) for (int d = 0; d < 3; d++) sum[d] += T->vertices[3 * ring[j] + d];
    double mid[3] = {sum[0] / nn, sum[1] / nn, sum[2] / nn}, dev[3];
    v_sub(mid, x, dev);
    double pn[3] = {0, 0, 0};
    for (int j = 0; j < nn; j++) {
      double a[3], b[3], tn[3];
      v_sub(T->vertices + 3 * ring[j], x, a);
      v_sub(T->vertices + 3 * ring[(j + 1) % nn], x, b);
      v_cross(a, b, tn);
      double l = v_norm(tn);
      for (int d = 0; d < 3; d++) { tn[d] /= l; pn[d] += tn[d]; }
    }
    double l = v_norm(pn); pn[0] /= l; pn[1] /= l; pn[2] /= l;
    T->patch_dist_eq[i] = v_dot(pn, dev);
  }
}

orc_celltype *orc_celltype_create(int model, int shape, double radius_lu, int min_triangles,
                                  double aspect_ratio, const long *inner_edges, int n_inner) {
  orc_celltype *T = (orc_celltype *)calloc(1, sizeof(orc_celltype));
  T->model = model;
  long nt; tri3 *t = make_shape(shape, radius_lu, min_triangles, aspect_ratio, &nt);
  long nv;
  dedupe(t, nt, &T->vertices, &nv, &T->triangles);
  free(t);
  T->nv = (int)nv; T->nt = (int)nt;
  mesh_inflate(T, 1.e-3);
  build_tables(T, inner_edges, n_inner);
  T->timescale = 1;
  return T;
}
void orc_celltype_destroy(orc_celltype *T) {
  if (!T) return;
  free(T->vertices); free(T->triangles); free(T->edges); free(T->edge_length_eq); free(T->edge_angle_eq);
  free(T->edge_bending_triangles); free(T->edge_bending_outer); free(T->triangle_area_eq);
  free(T->vertex_vertexes); free(T->vertex_n_vertexes); free(T->patch_dist_eq);
  free(T->inner_edges); free(T->inner_edge_length_eq); free(T);
}
double orc_mesh_surface(const orc_celltype *T) { /* MeshMetrics::getSurface = Nt*mean area */
  double s = 0; for (long t = 0; t < T->nt; t++) s += T->triangle_area_eq[t]; return s;
}

/* mechanics/cellMechanics.h:50-78 */
void orc_celltype_set_moduli(orc_celltype *T, const orc_params *P, double kLink, double kArea,
                             double kVolume, double kBend, double eta_m_si) {
  double persistenceLengthFine = 7.5e-9;
  double plc = persistenceLengthFine / P->dx;
  T->k_link = kLink * P->kBT_lbm / plc;
  double eqLength = 5e-7 / P->dx;
  T->k_bend = kBend * P->kBT_lbm / eqLength;
  double NfacesScaling = 1280.0 / T->nt;
  T->k_volume = kVolume * NfacesScaling * P->kBT_lbm / eqLength;
  T->k_area = kArea * NfacesScaling * P->kBT_lbm / (eqLength);
  T->eta_m = eta_m_si * P->dx / P->dt / P->df;
}

/* ======================================================================== */
/*                         MEMBRANE FORCES (a8, a9)                         */
/* ======================================================================== */
#define MaxCellVolumetricChange 0.01   /* config/constant_defaults.h:157-173 */
#define MaxCellSurfaceAreaChange 0.09
#define MaxCellBendingAngle 0.0555
#define MaxPLTBendingAngle 2.467
#define MaxCellPersistenceLength 9.0
#define FORCE_LIMIT 50.0

static inline void add3(double *dst, const double *s) { dst[0] += s[0]; dst[1] += s[1]; dst[2] += s[2]; }
static inline void sub3(double *dst, const double *s) { dst[0] -= s[0]; dst[1] -= s[1]; dst[2] -= s[2]; }

void orc_cell_forces(const orc_celltype *T, const double *pos, const double *vel, double *force,
                     double *comp, int flags) {
  const long nv = T->nv, nt = T->nt, ne = T->ne;
  double *f_vol = comp ? comp + 0 * 3 * nv : force, *f_area = comp ? comp + 1 * 3 * nv : force,
         *f_bend = comp ? comp + 2 * 3 * nv : force, *f_link = comp ? comp + 3 * 3 * nv : force,
         *f_visc = comp ? comp + 4 * 3 * nv : force, *f_inner = comp ? comp + 5 * 3 * nv : force;
  double *tri_area = (double *)malloc(sizeof(double) * (size_t)nt);
  double *tri_n = (double *)malloc(sizeof(double) * 3 * (size_t)nt);
  double volume = 0.0;
  /* per-triangle: mechanics/rbcHighOrderModel.cpp:56-98 == mechanics/pltSimpleModel.cpp:57-99 */
  for (long t = 0; t < nt; t++) {
    const long *tr = T->triangles + 3 * t;
    const double *v0 = pos + 3 * tr[0], *v1 = pos + 3 * tr[1], *v2 = pos + 3 * tr[2];
    const double v210 = v2[0] * v1[1] * v0[2];
    const double v120 = v1[0] * v2[1] * v0[2];
    const double v201 = v2[0] * v0[1] * v1[2];
    const double v021 = v0[0] * v2[1] * v1[2];
    const double v102 = v1[0] * v0[1] * v2[2];
    const double v012 = v0[0] * v1[1] * v2[2];
    volume += (-v210 + v120 + v201 - v021 - v102 + v012);
    double area, n[3];
    tri_area_unit_normal(v0, v1, v2, &area, n);
    tri_area[t] = area; memcpy(tri_n + 3 * t, n, 24);
    if (flags & 1) {
      const double areaRatio = (area - T->triangle_area_eq[t]) / T->triangle_area_eq[t];
      const double afm = T->k_area * (areaRatio + areaRatio / fabs(MaxCellSurfaceAreaChange - areaRatio * areaRatio));
      double centroid[3];
      centroid[0] = (v0[0] + v1[0] + v2[0]) / 3.0;
      centroid[1] = (v0[1] + v1[1] + v2[1]) / 3.0;
      centroid[2] = (v0[2] + v1[2] + v2[2]) / 3.0;
      for (int d = 0; d < 3; d++) {
        f_area[3 * tr[0] + d] += afm * (centroid[d] - v0[d]);
        f_area[3 * tr[1] + d] += afm * (centroid[d] - v1[d]);
        f_area[3 * tr[2] + d] += afm * (centroid[d] - v2[d]);
      }
    }
  }
  volume *= (1.0 / 6.0);
  /* volume force: rbcHighOrderModel.cpp:100-124 == pltSimpleModel.cpp:101-117 */
  if (flags & 2) {
    const double volume_frac = (volume - T->volume_eq) / T->volume_eq;
    const double volume_force = -T->k_volume * volume_frac / fabs(MaxCellVolumetricChange - volume_frac * volume_frac);
    for (long t = 0; t < nt; t++) {
      const long *tr = T->triangles + 3 * t;
      double lvf[3];
      for (int d = 0; d < 3; d++) lvf[d] = (volume_force * tri_n[3 * t + d]) * (tri_area[t] / T->area_mean_eq);
      add3(f_vol + 3 * tr[0], lvf); add3(f_vol + 3 * tr[1], lvf); add3(f_vol + 3 * tr[2], lvf);
    }
  }
  if (T->model == ORC_MODEL_RBC_HO) {
    /* per-vertex bending: rbcHighOrderModel.cpp:127-166 */
    if (flags & 4)
      for (long i = 0; i < nv; i++) {
        const int nn = T->vertex_n_vertexes[i];
        const long *ring = T->vertex_vertexes + 6 * i;
        const double *x = pos + 3 * i;
        double sum[3] = {0., 0., 0.};
        for (int j = 0; j < nn; j++) add3(sum, pos + 3 * ring[j]);
        double mid[3] = {sum[0] / nn, sum[1] / nn, sum[2] / nn}, dev[3];
        v_sub(mid, x, dev);
        double pn[3] = {0., 0., 0.};
        for (int j = 0; j < nn - 1; j++) {
          double a[3], b[3], tn[3];
          v_sub(pos + 3 * ring[j], x, a); v_sub(pos + 3 * ring[j + 1], x, b);
          v_cross(a, b, tn);
          double l = v_norm(tn); tn[0] /= l; tn[1] /= l; tn[2] /= l;
          add3(pn, tn);
        }
        {
          double a[3], b[3], tn[3];
          v_sub(pos + 3 * ring[nn - 1], x, a); v_sub(pos + 3 * ring[0], x, b);
          v_cross(a, b, tn);
          double l = v_norm(tn); tn[0] /= l; tn[1] /= l; tn[2] /= l;
          add3(pn, tn);
        }
        double l = v_norm(pn); pn[0] /= l; pn[1] /= l; pn[2] /= l;
        const double ndev = v_dot(pn, dev);
        const double dDev = (ndev - T->patch_dist_eq[i]) / T->edge_mean_eq;
        const double mag = T->k_bend * (dDev + dDev / fabs(MaxCellBendingAngle - dDev * dDev));
        double bf[3] = {mag * pn[0], mag * pn[1], mag * pn[2]};
        add3(f_bend + 3 * i, bf);
        double nbf[3] = {-bf[0] / nn, -bf[1] / nn, -bf[2] / nn};
        for (int j = 0; j < nn; j++) add3(f_bend + 3 * ring[j], nbf);
      }
    /* per-edge link (+ membrane viscosity if eta_m != 0): rbcHighOrderModel.cpp:169-204 */
    if (flags & 8)
      for (long e = 0; e < ne; e++) {
        const long e0 = T->edges[2 * e], e1 = T->edges[2 * e + 1];
        double ev[3]; v_sub(pos + 3 * e1, pos + 3 * e0, ev);
        const double el = v_norm(ev);
        double uv[3] = {ev[0] / el, ev[1] / el, ev[2] / el};
        const double ef = (el - T->edge_length_eq[e]) / T->edge_length_eq[e];
        const double fs = T->k_link * (ef + ef / fabs(MaxCellPersistenceLength - ef * ef));
        double fr[3] = {uv[0] * fs, uv[1] * fs, uv[2] * fs};
        add3(f_link + 3 * e0, fr); sub3(f_link + 3 * e1, fr);
        if (T->eta_m != 0.0) {
          double rv[3]; v_sub(vel + 3 * e1, vel + 3 * e0, rv);
          double pr = v_dot(rv, uv);
          double fv[3] = {T->eta_m * (pr * uv[0]), T->eta_m * (pr * uv[1]), T->eta_m * (pr * uv[2])};
          const double mag = v_norm(fv);
          if (mag > FORCE_LIMIT / 4.0) { double s = (FORCE_LIMIT / 4.0) / mag; fv[0] *= s; fv[1] *= s; fv[2] *= s; }
          add3(f_visc + 3 * e0, fv); sub3(f_visc + 3 * e1, fv);
        }
      }
  } else {
    /* PLT per-edge: link, viscosity (unconditional), dihedral bending: pltSimpleModel.cpp:120-183 */
    if (flags & (8 | 4))
      for (long e = 0; e < ne; e++) {
        const long e0 = T->edges[2 * e], e1 = T->edges[2 * e + 1];
        double ev[3]; v_sub(pos + 3 * e1, pos + 3 * e0, ev);
        const double el = sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
        double uv[3] = {ev[0] / el, ev[1] / el, ev[2] / el};
        if (flags & 8) {
          const double ef = (el - T->edge_length_eq[e]) / T->edge_length_eq[e];
          const double fs = T->k_link * (ef + ef / fabs(MaxCellPersistenceLength - ef * ef));
          double fr[3] = {uv[0] * fs, uv[1] * fs, uv[2] * fs};
          add3(f_link + 3 * e0, fr); sub3(f_link + 3 * e1, fr);
          double rv[3]; v_sub(vel + 3 * e1, vel + 3 * e0, rv);
          double pr = v_dot(rv, uv);
          double fv[3] = {T->eta_m * (pr * uv[0]), T->eta_m * (pr * uv[1]), T->eta_m * (pr * uv[2])};
          const double mag = v_norm(fv);
          if (mag > FORCE_LIMIT / 4.0) { double s = (FORCE_LIMIT / 4.0) / mag; fv[0] *= s; fv[1] *= s; fv[2] *= s; }
          add3(f_visc + 3 * e0, fv); sub3(f_visc + 3 * e1, fv);
        }
        if (flags & 4) {
          const long b0 = T->edge_bending_triangles[2 * e], b1 = T->edge_bending_triangles[2 * e + 1];
          const long *ta = T->triangles + 3 * b0, *tb = T->triangles + 3 * b1;
          double V1[3], V2[3];
          tri_unit_normal(pos + 3 * ta[0], pos + 3 * ta[1], pos + 3 * ta[2], V1);
          tri_unit_normal(pos + 3 * tb[0], pos + 3 * tb[1], pos + 3 * tb[2], V2);
          const double angle = angle_between_faces(V1, V2, uv);
          const double af = angle - T->edge_angle_eq[e];
          const double fm = T->k_bend * (af + af / fabs(MaxPLTBendingAngle - af * af));
          double bf[3];
          for (int d = 0; d < 3; d++) bf[d] = (fm * (V1[d] + V2[d])) * 0.5;
          add3(f_bend + 3 * e0, bf); add3(f_bend + 3 * e1, bf);
          sub3(f_bend + 3 * T->edge_bending_outer[2 * e], bf);
          sub3(f_bend + 3 * T->edge_bending_outer[2 * e + 1], bf);
        }
      }
    /* inner links: pltSimpleModel.cpp:186-205 */
    if (flags & 16)
      for (long e = 0; e < T->nie; e++) {
        const long e0 = T->inner_edges[2 * e], e1 = T->inner_edges[2 * e + 1];
        double ev[3]; v_sub(pos + 3 * e1, pos + 3 * e0, ev);
        const double el = sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
        double uv[3] = {ev[0] / el, ev[1] / el, ev[2] / el};
        const double ef = (el - T->inner_edge_length_eq[e]) / T->inner_edge_length_eq[e];
        const double fs = T->k_link * 5.0 * ef;
        double fr[3] = {uv[0] * fs, uv[1] * fs, uv[2] * fs};
        add3(f_inner + 3 * e0, fr); sub3(f_inner + 3 * e1, fr);
      }
  }
  free(tri_area); free(tri_n);
}

/* ======================================================================== */
/*                                   IBM                                    */
/* ======================================================================== */

/* interpolationCoefficientsPhi2, core/immersedBoundaryMethod.h:62-138.
 * One global block: "contained in the block's bounding box" becomes "inside
 * the domain, or wrapped if that axis is periodic" (the reference reaches the
 * same nodes through envelope copies of the particle). long(x+0.5) truncates
 * toward zero exactly as plint(position+0.5) does (:86). */
int orc_phi2_stencil(const orc_lattice *L, const double pos[3], long nodes[8], double weights[8]) {
  const int dims[3] = {L->nx, L->ny, L->nz};
  long center[3];
  /* plint(position+0.5) (:86) truncates; it equals floor on the block-relative coordinates (>= 0) the
   * reference applies it to.  floor is used so that an unwrapped periodic image at negative x picks the
   * nodes of its wrapped position. */
  for (int d = 0; d < 3; d++) center[d] = (long)floor(pos[d] + 0.5);
  int cnt = 0; double total = 0;
  for (int dx = -1; dx < 2; dx++)
    for (int dy = -1; dy < 2; dy++)
      for (int dz = -1; dz < 2; dz++) {
        long p[3] = {center[0] + dx, center[1] + dy, center[2] + dz};
        long w[3]; int ok = 1;
        for (int d = 0; d < 3; d++) {
          w[d] = p[d];
          if (p[d] < 0 || p[d] >= dims[d]) {
            if (L->periodic[d]) w[d] = ((p[d] % dims[d]) + dims[d]) % dims[d]; else ok = 0;
          }
        }
        if (!ok) continue;
        double ph[3];
        for (int d = 0; d < 3; d++) { double x = fabs(pos[d] - (double)p[d]); x = 1.0 - x; ph[d] = x > 0.0 ? x : 0.0; }
        double weight = ph[0] * ph[1] * ph[2];
        if (weight == 0.0) continue;
        long node = w[2] + (long)L->nz * (w[1] + (long)L->ny * w[0]);
        if (L->mask[node]) continue;
        total += weight;
        weights[cnt] = weight; nodes[cnt] = node; cnt++;
      }
  const double coeff = 1.0 / total;
  for (int k = 0; k < cnt; k++) weights[k] *= coeff;
  return cnt;
}

/* ======================================================================== */
/*                                SIMULATION                                */
/* ======================================================================== */
orc_sim *orc_sim_create(orc_lattice *L, const orc_params *P) {
  orc_sim *S = (orc_sim *)calloc(1, sizeof(orc_sim));
  S->L = L; S->P = *P;
  S->particle_velocity_timescale = 1;
  S->force_limit_enabled = 1;
  S->rep_enabled = 0; S->rep_timescale = 1;
  S->brep_enabled = 0; S->brep_timescale = 1;
  return S;
}
void orc_sim_destroy(orc_sim *S) {
  if (!S) return;
  free(S->particles); free(S->st_nodes); free(S->st_w); free(S->st_n); free(S->dead); free(S);
}
int orc_sim_add_type(orc_sim *S, orc_celltype *T) { S->types[S->ntypes] = T; S->ncells[S->ntypes] = 0; return S->ntypes++; }
long orc_sim_type_offset(const orc_sim *S, int type) {
  long off = 0; for (int t = 0; t < type; t++) off += S->ncells[t] * S->types[t]->nv; return off;
}

/* rotateTriangularMeshXYZ, io/readPositionsBloodCells.cpp:40-111 (literal index pattern) */
static void rotation_xyz(double alpha, double beta, double gamma, double a[3][3]) {
  double b[3][3], c[3][3];
  a[0][0] = 1; a[0][1] = 0; a[0][2] = 0;
  a[1][0] = 0; a[1][1] = cos(alpha); a[1][2] = sin(alpha);
  a[2][0] = 0; a[2][1] = -sin(alpha); a[2][2] = cos(alpha);
  b[0][0] = cos(beta); b[0][1] = 0; b[0][2] = -sin(beta);
  b[1][0] = 0; b[1][1] = 1; b[1][2] = 0;
  b[2][0] = sin(beta); b[2][1] = 0; b[2][2] = cos(beta);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { c[i][j] = 0; for (int k = 0; k < 3; k++) c[i][j] += a[k][j] * b[i][k]; }
  b[0][0] = cos(gamma); b[0][1] = sin(gamma); b[0][2] = 0;
  b[1][0] = -sin(gamma); b[1][1] = cos(gamma); b[1][2] = 0;
  b[2][0] = 0; b[2][1] = 0; b[2][2] = 1;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { a[i][j] = 0; for (int k = 0; k < 3; k++) a[i][j] += c[k][j] * b[i][k]; }
}

static void bbox_centre(const double *v, long nv, double c[3]) {
  double lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
  for (long i = 1; i < nv; i++) for (int d = 0; d < 3; d++) { if (v[3 * i + d] < lo[d]) lo[d] = v[3 * i + d]; if (v[3 * i + d] > hi[d]) hi[d] = v[3 * i + d]; }
  for (int d = 0; d < 3; d++) c[d] = (hi[d] + lo[d]) * 0.5;
}

static int node_is_boundary_abs(const orc_lattice *L, long x, long y, long z, int *inside) {
  long p[3] = {x, y, z}; const int dims[3] = {L->nx, L->ny, L->nz};
  *inside = 1;
  for (int d = 0; d < 3; d++)
    if (p[d] < 0 || p[d] >= dims[d]) { if (L->periodic[d]) p[d] = ((p[d] % dims[d]) + dims[d]) % dims[d]; else { *inside = 0; return 0; } }
  return L->mask[p[2] + (long)L->nz * (p[1] + (long)L->ny * p[0])];
}

/* io/readPositionsBloodCells.cpp:113-169 (meshRotation + positionCellInParticleField)
 * and :303-353: mesh centred on its bounding-box centre, rotated about that
 * centre (X,Y,Z order), vertex = centre + meshVertex; a vertex is rejected when
 * its nearest node, or any node within denyLayerSize of it, is a boundary; a
 * cell with a rejected vertex is incomplete and is dropped (:353). */
int orc_sim_add_cell(orc_sim *S, int type, const double centre_lu[3], const double angles[3],
                     double min_dist_from_solid_um) {
  const orc_celltype *T = S->types[type];
  const long nv = T->nv;
  double *m = (double *)malloc(sizeof(double) * 3 * (size_t)nv);
  double c0[3]; bbox_centre(T->vertices, nv, c0);
  for (long i = 0; i < nv; i++) for (int d = 0; d < 3; d++) m[3 * i + d] = T->vertices[3 * i + d] - c0[d];
  double mc[3]; bbox_centre(m, nv, mc);
  double R[3][3]; rotation_xyz(angles[0], angles[1], angles[2], R);
  for (long i = 0; i < nv; i++) {
    double x[3] = {m[3 * i] + -1.0 * mc[0], m[3 * i + 1] + -1.0 * mc[1], m[3 * i + 2] + -1.0 * mc[2]}, r[3];
    for (int a = 0; a < 3; a++) { r[a] = 0; for (int b = 0; b < 3; b++) r[a] += R[a][b] * x[b]; }
    for (int d = 0; d < 3; d++) m[3 * i + d] = r[d] + mc[d];
  }
  int deny = (int)((min_dist_from_solid_um * 1e-6) / S->P.dx);
  int ok = 1;
  for (long i = 0; i < nv && ok; i++) {
    double v[3] = {centre_lu[0] + m[3 * i], centre_lu[1] + m[3 * i + 1], centre_lu[2] + m[3 * i + 2]};
    long n[3] = {(long)floor(v[0] + 0.5), (long)floor(v[1] + 0.5), (long)floor(v[2] + 0.5)}; /* int(vertex+0.5), :135 */
    int inside;
    if (node_is_boundary_abs(S->L, n[0], n[1], n[2], &inside)) { ok = 0; break; }
    for (int px = -deny; px <= deny && ok; px++) for (int py = -deny; py <= deny && ok; py++) for (int pz = -deny; pz <= deny; pz++)
      if (node_is_boundary_abs(S->L, n[0] + px, n[1] + py, n[2] + pz, &inside)) { ok = 0; break; }
  }
  if (ok) {
    /* insert at the end of this type's block (cell-major, types in order) */
    long off = orc_sim_type_offset(S, type) + S->ncells[type] * nv;
    long total_cells = 0; for (int t = 0; t < S->ntypes; t++) total_cells += S->ncells[t];
    S->particles = (orc_particle *)realloc(S->particles, sizeof(orc_particle) * (size_t)(S->np + nv));
    memmove(S->particles + off + nv, S->particles + off, sizeof(orc_particle) * (size_t)(S->np - off));
    for (long i = 0; i < nv; i++) {
      orc_particle *p = S->particles + off + i;
      memset(p, 0, sizeof(*p));
      for (int d = 0; d < 3; d++) p->position[d] = centre_lu[d] + m[3 * i + d];
      p->cellId = total_cells; p->vertexId = (unsigned short)i; p->celltype = (unsigned char)type;
    }
    S->dead = (unsigned char *)realloc(S->dead, (size_t)(S->np + nv));
    memmove(S->dead + off + nv, S->dead + off, (size_t)(S->np - off));
    memset(S->dead + off, 0, (size_t)nv);
    S->np += nv; S->ncells[type]++;
    S->st_nodes = (long *)realloc(S->st_nodes, sizeof(long) * 8 * (size_t)S->np);
    S->st_w = (double *)realloc(S->st_w, sizeof(double) * 8 * (size_t)S->np);
    S->st_n = (int *)realloc(S->st_n, sizeof(int) * (size_t)S->np);
    memset(S->st_n, 0, sizeof(int) * (size_t)S->np);
  }
  free(m);
  return ok;
}

/* HemoCellParticleField::spreadParticleForce, core/hemoCellParticleField.cpp:841-863 */
void orc_sim_spread(orc_sim *S) {
  orc_lattice *L = S->L;
  /* with more than one thread (CPU-baseline timing only) the additions become atomic and their order is no
   * longer the reference's; the parity tests run this loop on one thread */
  const int par = L->nthreads > 1;
#pragma omp parallel for num_threads(L->nthreads) schedule(static) if (par)
  for (long p = 0; p < S->np; p++) {
    orc_particle *pt = S->particles + p;
    long *nodes = S->st_nodes + 8 * p; double *w = S->st_w + 8 * p;
    if (S->dead[p]) { S->st_n[p] = 0; continue; }   /* removed from the particle list (removeParticles, :304-321) */
    S->st_n[p] = orc_phi2_stencil(L, pt->position, nodes, w);
    if (S->force_limit_enabled) {
      const double mag = v_norm(pt->force);
      if (mag > S->P.f_limit) { double s = S->P.f_limit / mag; pt->force[0] *= s; pt->force[1] *= s; pt->force[2] *= s; }
    }
    for (int j = 0; j < S->st_n[p]; j++)
      for (int d = 0; d < 3; d++) {
        const double add = ((pt->force_repulsion[d] + pt->force[d]) * w[j]);
        if (par) {
#pragma omp atomic
          L->force[3 * nodes[j] + d] += add;
        } else L->force[3 * nodes[j] + d] += add;
      }
  }
}

/* HemoCellParticleField::interpolateFluidVelocity, core/hemoCellParticleField.cpp:819-839:
 * reuses the stencil cached by the spread of the same iteration (:827) */
void orc_sim_interpolate(orc_sim *S) {
#pragma omp parallel for num_threads(S->L->nthreads) schedule(static) if (S->L->nthreads > 1)
  for (long p = 0; p < S->np; p++) {
    orc_particle *pt = S->particles + p;
    if (S->dead[p]) continue;
    double vel[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < S->st_n[p]; j++) {
      double rho, u[3];
      orc_node_rho_u(S->L, S->st_nodes[8 * p + j], &rho, u);
      for (int d = 0; d < 3; d++) vel[d] += (u[d] * S->st_w[8 * p + j]);
    }
    for (int d = 0; d < 3; d++) pt->v[d] = vel[d];
  }
}

static void delete_cell(orc_sim *S, int type, long cell) {
  const long nv = S->types[type]->nv;
  long off = orc_sim_type_offset(S, type) + cell * nv;
  memmove(S->particles + off, S->particles + off + nv, sizeof(orc_particle) * (size_t)(S->np - off - nv));
  memmove(S->st_nodes + 8 * off, S->st_nodes + 8 * (off + nv), sizeof(long) * 8 * (size_t)(S->np - off - nv));
  memmove(S->st_w + 8 * off, S->st_w + 8 * (off + nv), sizeof(double) * 8 * (size_t)(S->np - off - nv));
  memmove(S->st_n + off, S->st_n + off + nv, sizeof(int) * (size_t)(S->np - off - nv));
  memmove(S->dead + off, S->dead + off + nv, (size_t)(S->np - off - nv));
  S->np -= nv; S->ncells[type]--; S->cells_deleted++;
}

/* HemoCellParticle::advance (core/hemoCellParticle.h:188-203, Euler) +
 * HemoCellParticleField::advanceParticles (core/hemoCellParticleField.cpp:566-588): every particle moves; one whose
 * nearest node is a boundary gets tag 1 and removeParticles(1) (:584, :304-321) takes it out of the list.  With
 * deletion_mode 1 the whole cell goes instead. */
void orc_sim_advance(orc_sim *S) {
#pragma omp parallel for num_threads(S->L->nthreads) schedule(static) if (S->L->nthreads > 1)
  for (long p = 0; p < S->np; p++) {
    orc_particle *pt = S->particles + p;
    if (S->dead[p]) continue;
    for (int d = 0; d < 3; d++) pt->position[d] += pt->v[d];
  }
  for (int t = 0; t < S->ntypes; t++) {
    const long nv = S->types[t]->nv;
    for (long c = 0; c < S->ncells[t]; c++) {
      long off = orc_sim_type_offset(S, t) + c * nv;
      int tagged = 0;
      for (long i = 0; i < nv; i++) {
        if (S->dead[off + i]) continue;
        const double *x = S->particles[off + i].position;
        long nx = (long)floor(x[0] + 0.5), ny = (long)floor(x[1] + 0.5), nz = (long)floor(x[2] + 0.5);
        int inside;
        if (node_is_boundary_abs(S->L, nx, ny, nz, &inside)) {
          tagged = 1;
          if (S->deletion_mode == 0) { S->dead[off + i] = 1; S->particles_deleted++; } else break;
        }
      }
      if (tagged && S->deletion_mode != 0) { delete_cell(S, t, c); c--; }
    }
  }
}

static int cell_is_complete(const orc_sim *S, long off, long nv) {
  for (long i = 0; i < nv; i++) if (S->dead[off + i]) return 0;
  return 1;
}

/* HemoCellParticleField::deleteIncompleteCells, core/hemoCellParticleField.cpp:512-553 */
long orc_sim_delete_incomplete_cells(orc_sim *S) {
  long removed = 0;
  for (int t = 0; t < S->ntypes; t++) {
    const long nv = S->types[t]->nv;
    for (long c = 0; c < S->ncells[t]; c++) {
      const long off = orc_sim_type_offset(S, t) + c * nv;
      if (!cell_is_complete(S, off, nv)) { delete_cell(S, t, c); c--; removed++; }
    }
  }
  return removed;
}
void orc_sim_get_alive(const orc_sim *S, unsigned char *alive) { for (long p = 0; p < S->np; p++) alive[p] = S->dead[p] ? 0 : 1; }

/* HemoCellParticleField::applyConstitutiveModel, core/hemoCellParticleField.cpp:633-675 */
void orc_sim_mechanics(orc_sim *S, int forced) {
  for (int t = 0; t < S->ntypes; t++) {
    const orc_celltype *T = S->types[t];
    if (!(S->iter % T->timescale == 0 || forced)) continue;
    const long nv = T->nv;
    const long off = orc_sim_type_offset(S, t);
    /* cells are independent: one cell per thread changes no result */
#pragma omp parallel num_threads(S->L->nthreads) if (S->L->nthreads > 1)
    {
      double *pos = (double *)malloc(sizeof(double) * 3 * (size_t)nv), *vel = (double *)malloc(sizeof(double) * 3 * (size_t)nv),
             *frc = (double *)malloc(sizeof(double) * 3 * (size_t)nv);
#pragma omp for schedule(static)
      for (long c = 0; c < S->ncells[t]; c++) {
        orc_particle *cp = S->particles + off + c * nv;
        if (!cell_is_complete(S, off + c * nv, nv)) {
          /* every particle of the type has its force zeroed (:660-667), but only complete cells reach ParticleMechanics (:634-652, :669) */
          for (long i = 0; i < nv; i++) for (int d = 0; d < 3; d++) cp[i].force[d] = 0.0;
          continue;
        }
        for (long i = 0; i < nv; i++) for (int d = 0; d < 3; d++) { pos[3 * i + d] = cp[i].position[d]; vel[3 * i + d] = cp[i].v[d]; frc[3 * i + d] = 0.0; }
        orc_cell_forces(T, pos, vel, frc, NULL, 0x1f);
        for (long i = 0; i < nv; i++) for (int d = 0; d < 3; d++) cp[i].force[d] = frc[3 * i + d];
      }
      free(pos); free(vel); free(frc);
    }
  }
}

/* accessors for the ctypes test harness */
void orc_sim_get(const orc_sim *S, int what, double *out) {
  for (long p = 0; p < S->np; p++) {
    const orc_particle *pt = S->particles + p;
    const double *src = what == 0 ? pt->position : what == 1 ? pt->v : what == 2 ? pt->force : pt->force_repulsion;
    out[3 * p] = src[0]; out[3 * p + 1] = src[1]; out[3 * p + 2] = src[2];
  }
}
void orc_sim_set(orc_sim *S, int what, const double *in) {
  for (long p = 0; p < S->np; p++) {
    orc_particle *pt = S->particles + p;
    double *dst = what == 0 ? pt->position : what == 1 ? pt->v : what == 2 ? pt->force : pt->force_repulsion;
    dst[0] = in[3 * p]; dst[1] = in[3 * p + 1]; dst[2] = in[3 * p + 2];
  }
}
/* helper/hemoCellStretch.cpp:63-78: sv.force -/+= ex_force on selected vertices */
void orc_sim_add_vertex_force(orc_sim *S, long particle, const double f[3]) {
  for (int d = 0; d < 3; d++) S->particles[particle].force[d] += f[d];
}

/* HemoCellParticleField::applyRepulsionForce, core/hemoCellParticleField.cpp:677-743, with the particle grid of
 * update_pg (:137-168): particles binned by nearest node; for every bin the reference visits the bin itself
 * (ordered pairs, so every same-bin pair is applied twice) and 13 of its 26 neighbours (each adjacent pair of bins
 * once).  One global block: bins wrap in periodic directions and the separation of a pair is taken to its minimum
 * image (what the reference's shifted periodic envelope copies amount to). */
void orc_sim_repulsion(orc_sim *S, double r_const, double r_cutoff) {
  const orc_lattice *L = S->L;
  const int dims[3] = {L->nx, L->ny, L->nz};
  const long nb = (long)L->nx * L->ny * L->nz;
  long *head = (long *)malloc(sizeof(long) * (size_t)nb), *tail = (long *)malloc(sizeof(long) * (size_t)nb), *next = (long *)malloc(sizeof(long) * (size_t)(S->np > 0 ? S->np : 1));
  for (long b = 0; b < nb; b++) head[b] = tail[b] = -1;
  for (long p = 0; p < S->np; p++) {
    orc_particle *pt = S->particles + p;
    pt->force_repulsion[0] = pt->force_repulsion[1] = pt->force_repulsion[2] = 0.;
    long c[3]; int ok = S->dead[p] ? 0 : 1;   /* a removed particle is in no bin */
    for (int d = 0; d < 3; d++) {
      c[d] = (long)floor(pt->position[d] + 0.5);
      if (c[d] < 0 || c[d] >= dims[d]) { if (L->periodic[d]) c[d] = ((c[d] % dims[d]) + dims[d]) % dims[d]; else ok = 0; }
    }
    next[p] = -1;
    if (!ok || S->dead[p]) continue;
    const long b = c[2] + (long)L->nz * (c[1] + (long)L->ny * c[0]);
    if (head[b] < 0) head[b] = p; else next[tail[b]] = p;   /* insertion order = particle order, as particle_grid[index][k] */
    tail[b] = p;
  }
  static const int half[14][3] = {{0, 0, 0}, {0, 0, 1}, {0, 1, 0}, {0, 1, 1}, {1, -1, -1}, {1, -1, 0}, {1, -1, 1}, {1, 0, -1}, {1, 0, 0},
                                  {1, 0, 1}, {1, 1, -1}, {1, 1, 0}, {1, 1, 1}, {0, 1, -1}};
  for (int x = 0; x < L->nx; x++) for (int y = 0; y < L->ny; y++) for (int z = 0; z < L->nz; z++) {
    const long lb = z + (long)L->nz * (y + (long)L->ny * x);
    if (head[lb] < 0) continue;
    for (int h = 0; h < 14; h++) {
      long n[3] = {x + half[h][0], y + half[h][1], z + half[h][2]}; int ok = 1;
      for (int d = 0; d < 3; d++) {
        if (n[d] < 0) { if (L->periodic[d]) n[d] += dims[d]; else ok = 0; }
        else if (n[d] >= dims[d]) { if (L->periodic[d]) n[d] -= dims[d]; else ok = 0; }
      }
      if (!ok) continue;
      const long nbn = n[2] + (long)L->nz * (n[1] + (long)L->ny * n[0]);
      for (long i = head[lb]; i >= 0; i = next[i])
        for (long j = head[nbn]; j >= 0; j = next[j]) {
          orc_particle *lp = S->particles + i, *np_ = S->particles + j;
          if (np_ == lp) continue;
          if (lp->cellId == np_->cellId && lp->celltype == np_->celltype) continue;
          double dv[3];
          /* positions are not re-wrapped when a cell crosses a periodic face (the reference shifts them by the
           * domain length when they change block): take the minimum image of the separation */
          for (int d = 0; d < 3; d++) {
            dv[d] = lp->position[d] - np_->position[d];
            if (L->periodic[d]) dv[d] = dv[d] - (double)dims[d] * rint(dv[d] / (double)dims[d]);
          }
          const double distance = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
          if (distance < r_cutoff) {
            for (int d = 0; d < 3; d++) {
              const double rfm = r_const * (1 / (distance / r_cutoff)) * (dv[d] / distance);
              lp->force_repulsion[d] = lp->force_repulsion[d] + rfm;
              np_->force_repulsion[d] = np_->force_repulsion[d] - rfm;
            }
          }
        }
    }
  }
  free(head); free(tail); free(next);
}

/* Boundary particles: HemoCellParticleField::populateBoundaryParticles (core/hemoCellParticleField.cpp:865-890) makes
 * one of every boundary node that has a non-boundary node among its 26 neighbours; applyBoundaryRepulsionForce
 * (:891-918) lets each push the vertices binned (update_pg, nearest node) in the 27 bins around it:
 *   force_repulsion += k * (1 / (dist / cutoff)) * (dv / dist)   for dist < cutoff, dv = x_vertex - x_node.
 * Restated per vertex: the 27 nodes around the vertex's bin in ascending (x, y, z) order, which is the order in
 * which the reference's boundaryParticles list (built x-major) reaches that vertex.  One global block: nodes wrap in
 * periodic directions (the reference's loops run over a block with its periodic envelope).  force_repulsion is
 * only ever zeroed by applyRepulsionForce (:703), so without vertex-vertex repulsion it accumulates, as it does
 * in the reference. */
static int is_boundary_particle(const orc_lattice *L, long x, long y, long z) {
  int inside;
  if (!node_is_boundary_abs(L, x, y, z, &inside) || !inside) return 0;
  for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) for (int c = -1; c <= 1; c++) {
    int in2;
    const int m = node_is_boundary_abs(L, x + a, y + b, z + c, &in2);
    if (in2 && !m) return 1;
  }
  return 0;
}
void orc_sim_boundary_repulsion(orc_sim *S, double br_const, double br_cutoff) {
  const orc_lattice *L = S->L;
  const int dims[3] = {L->nx, L->ny, L->nz};
  for (long p = 0; p < S->np; p++) {
    orc_particle *pt = S->particles + p;
    long c[3]; int ok = 1;
    if (S->dead[p]) continue;
    for (int d = 0; d < 3; d++) {
      c[d] = (long)floor(pt->position[d] + 0.5);
      if ((c[d] < 0 || c[d] >= dims[d]) && !L->periodic[d]) ok = 0;   /* not in the particle grid (:158-161) */
    }
    if (!ok) continue;
    for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) for (int e = -1; e <= 1; e++) {
      const long n[3] = {c[0] + a, c[1] + b, c[2] + e};
      if (!is_boundary_particle(L, n[0], n[1], n[2])) continue;
      double dv[3]; for (int d = 0; d < 3; d++) dv[d] = pt->position[d] - (double)n[d];
      const double distance = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
      if (distance < br_cutoff)
        for (int d = 0; d < 3; d++) {
          const double rfm = br_const * (1 / (distance / br_cutoff)) * (dv[d] / distance);
          pt->force_repulsion[d] = pt->force_repulsion[d] + rfm;
        }
    }
  }
}

/* HemoCell::iterate, core/hemoCell.cpp:299-376, followed by the driver's
 * setExternalVector(body force) (examples/pipeflow/pipeflow.cpp:144-146) */
void orc_sim_iterate(orc_sim *S) {
  if (S->rep_enabled && S->iter % S->rep_timescale == 0) orc_sim_repulsion(S, S->rep_const, S->rep_cutoff);   /* :307-309 */
  if (S->brep_enabled && S->iter % S->brep_timescale == 0) orc_sim_boundary_repulsion(S, S->brep_const, S->brep_cutoff);   /* :310-312 */
  orc_sim_spread(S);                                            /* :313 */
  orc_collide_stream(S->L);                                     /* :317 */
  if (S->iter % S->particle_velocity_timescale == 0) orc_sim_interpolate(S); /* :327-332 */
  orc_sim_advance(S);                                           /* :342 */
  orc_sim_mechanics(S, 0);                                      /* :345 */
  orc_lattice_set_force_uniform(S->L, S->body_force);           /* :369-371 + driver */
  for (int r = 0; r < S->n_regions; r++) orc_lattice_set_force_box(S->L, S->region_box[r], S->region_force[r]);
  S->iter++;                                                    /* :374 */
}
