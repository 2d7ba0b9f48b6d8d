// Ellipsoid force-bias packing on the GPU: cells to a target hematocrit in a periodic box.
//
// Replaces (file:line in the HemoCell tree, all under tools/packCells/):
//   packing.h:265-343    Packing::init           -> hc_packing_create (host scalars, first calc_forces)
//   packing.h:345-368    Packing::iterate        -> one queued iteration: pk_motion, pk_bin, pk_list, pk_pair, pk_sum, pk_control
//   packing.h:399-428    calc_motion             -> pk_motion
//   packing.h:370-397, :430-495  calc_forces, force_part, force_all -> pk_bin + pk_list (which pairs), pk_pair, pk_sum
//   packing.h:108-144    calc_forces(e, ei, ej)  -> pair_eval
//   packing.h:697-764    zeroin                  -> root_search (capped at ROOT_CAP evaluations)
//   ellipsoid.h:303-405  BinaryEllipsoidSystem   -> contact_setup, Contact
//   geometry.h           vector3, matrix33, Quaternion, in the reference's operand order
//
// Mapping (DESIGN §4 "packing"): every particle keeps a list of its partners in ascending index (pk_list: one wave per
// particle scans all particles 64 at a time and appends by ballot prefix, so the order needs no sort); pk_pair runs one
// thread per list slot and stores that particle's own force and torque increment; pk_sum adds a particle's slots in order.
// A pair therefore is evaluated twice, once from each side, by the same function on the same operands (A is the higher
// index on both sides), which makes the two increments bitwise opposite without any floating-point atomic.  The control
// scalars live in one device block (Ctl); every kernel of an iteration returns at once when finished, error or grow is
// set, so hc_packing_run queues its iterations blind and waits once.
//
// Walls (hc_packing_set_walls; this back end's own, the reference packs periodic boxes only): a particle near a wall gets one
// more partner, its mirror image across the wall's tangent plane (wall_eval), evaluated by pk_wall and added by pk_sum after
// the partner slots.  The wall's signed distance comes from a field built once on the device (pk_edt_*), sampled trilinearly
// (wall_sample).  pk_motion, pk_pair and pk_sum are templates on WALLS; without walls the <false> instances run, whose code
// is that of the periodic packing, and pk_wall is not launched.
#include "common.h"
#include <cmath>

namespace {

constexpr int ROOT_CAP = 256;   // evaluations of f_AB_d per pair; the reference's loop is unbounded
constexpr int NFIG = 16;        // packing.h:151

struct Ctl {
  double Douter, Douter2, Relax, Dinner, Force_step, Pactual, DensityNominal;
  int Nsf, doExit, finished, steps, error, grow, maxeval, maxcount;
};

struct V3 { double v[3]; };
struct M3 { double m[3][3]; };
struct Q4 { double s; V3 p; };

#define PK_FN __device__ __forceinline__

PK_FN double dot3(const V3 &a, const V3 &b) { return a.v[0] * b.v[0] + a.v[1] * b.v[1] + a.v[2] * b.v[2]; }   // geometry.h:141
PK_FN V3 cross3(const V3 &a, const V3 &b) {   // geometry.h:154
  V3 r;
  r.v[0] = a.v[1] * b.v[2] - a.v[2] * b.v[1];
  r.v[1] = a.v[2] * b.v[0] - a.v[0] * b.v[2];
  r.v[2] = a.v[0] * b.v[1] - a.v[1] * b.v[0];
  return r;
}
PK_FN V3 vmul(const V3 &a, double d) { V3 r; r.v[0] = a.v[0] * d; r.v[1] = a.v[1] * d; r.v[2] = a.v[2] * d; return r; }
PK_FN V3 normalised(const V3 &a) {   // norm(), geometry.h:157-161, with its shortcut
  const double sp = dot3(a, a);
  if (fabs(sp - 1) < 1e-10) return a;
  return vmul(a, 1 / sqrt(sp));
}
PK_FN M3 mmul(const M3 &a, const M3 &b) {   // geometry.h:186-198
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return r;
}
PK_FN M3 mscale(const M3 &a, double d) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] * d;
  return r;
}
PK_FN M3 madd(const M3 &a, const M3 &b) {
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] + b.m[i][j];
  return r;
}
PK_FN V3 mvec(const M3 &a, const V3 &x) {   // geometry.h:302-308
  V3 r;
#pragma unroll
  for (int i = 0; i < 3; i++) r.v[i] = a.m[i][0] * x.v[0] + a.m[i][1] * x.v[1] + a.m[i][2] * x.v[2];
  return r;
}
PK_FN M3 adj3(const M3 &a) {   // geometry.h:321-333
  M3 r;
  r.m[0][0] = a.m[1][1] * a.m[2][2] - a.m[1][2] * a.m[2][1];
  r.m[0][1] = a.m[1][2] * a.m[2][0] - a.m[1][0] * a.m[2][2];
  r.m[0][2] = a.m[1][0] * a.m[2][1] - a.m[1][1] * a.m[2][0];
  r.m[1][0] = a.m[0][2] * a.m[2][1] - a.m[2][2] * a.m[0][1];
  r.m[1][1] = a.m[0][0] * a.m[2][2] - a.m[0][2] * a.m[2][0];
  r.m[1][2] = a.m[0][1] * a.m[2][0] - a.m[0][0] * a.m[2][1];
  r.m[2][0] = a.m[0][1] * a.m[1][2] - a.m[0][2] * a.m[1][1];
  r.m[2][1] = a.m[1][0] * a.m[0][2] - a.m[0][0] * a.m[1][2];
  r.m[2][2] = a.m[1][1] * a.m[0][0] - a.m[1][0] * a.m[0][1];
  return r;
}
PK_FN double det3(const M3 &a) {   // geometry.h:334-337
  return a.m[0][0] * a.m[1][1] * a.m[2][2] + a.m[1][0] * a.m[2][1] * a.m[0][2] + a.m[2][0] * a.m[0][1] * a.m[1][2] -
         a.m[0][2] * a.m[1][1] * a.m[2][0] - a.m[0][0] * a.m[1][2] * a.m[2][1] - a.m[0][1] * a.m[1][0] * a.m[2][2];
}
PK_FN double vmv3(const M3 &c, const V3 &x) {   // geometry.h:351-360
  double w = c.m[0][0] * x.v[0] * x.v[0] + c.m[1][1] * x.v[1] * x.v[1] + c.m[2][2] * x.v[2] * x.v[2];
  w += c.m[0][1] * x.v[0] * x.v[1];
  w += c.m[0][2] * x.v[0] * x.v[2];
  w += c.m[1][0] * x.v[1] * x.v[0];
  w += c.m[1][2] * x.v[1] * x.v[2];
  w += c.m[2][0] * x.v[2] * x.v[0];
  w += c.m[2][1] * x.v[2] * x.v[1];
  return w;
}
// Quaternion(s, p): the constructor renormalises beyond 1e-10 (geometry.h:386, 406-414); the probe's input quaternions
PK_FN Q4 quat_make(double s, const V3 &p) {
  Q4 q; q.s = s; q.p = p;
  double sp = q.s * q.s + dot3(q.p, q.p);
  if (fabs(sp - 1) > 1e-10) {
    sp = 1 / sqrt(sp);
    q.s *= sp;
    q.p = vmul(q.p, sp);
  }
  return q;
}
// The rotation of a step, (cp2, sp2 fu) (packing.h:423), always brought to unit norm.  The reference's constructor leaves a
// squared norm within 1e-10 of 1 as it is, and rotate() keeps what is left in the product for good (deviation 10).
PK_FN Q4 quat_unit(double s, const V3 &p) {
  Q4 q;
  const double sp = 1 / sqrt(s * s + dot3(p, p));
  q.s = s * sp;
  q.p = vmul(p, sp);
  return q;
}
// t *= q, geometry.h:400-405 (no renormalisation)
PK_FN Q4 quat_mul(const Q4 &t, const Q4 &q) {
  Q4 r;
  r.s = t.s * q.s - dot3(t.p, q.p);
  const V3 c = cross3(t.p, q.p);
#pragma unroll
  for (int k = 0; k < 3; k++) r.p.v[k] = (t.s * q.p.v[k] + q.s * t.p.v[k]) - c.v[k];
  return r;
}
// countQ(), geometry.h:424-428: 2 (p p^T - s skew(p) + (s^2 - 1/2) I), with the zero entries of skew and I multiplied through
PK_FN M3 quat_matrix(const Q4 &q) {
  const double sk[3][3] = {{0, -q.p.v[2], q.p.v[1]}, {q.p.v[2], 0, -q.p.v[0]}, {-q.p.v[1], q.p.v[0], 0}};
  const double c = q.s * q.s - 0.5;
  M3 r;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) r.m[i][j] = 2 * ((q.p.v[i] * q.p.v[j] - q.s * sk[i][j]) + c * (i == j ? 1.0 : 0.0));
  return r;
}
// countX_m1 / countX_12 (ellipsoid.h:81-98): transp(Q) * diag(d) * Q, the diagonal matrix multiplied in full
PK_FN M3 shape_matrix(const M3 &Q, double d0, double d1, double d2) {
  M3 o, t;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { o.m[i][j] = 0; t.m[i][j] = Q.m[j][i]; }
  o.m[0][0] = d0; o.m[1][1] = d1; o.m[2][2] = d2;
  return mmul(mmul(t, o), Q);
}
PK_FN bool sphere(const double r[3]) { return fabs(r[0] - r[2]) < 1e-5 && fabs(r[0] - r[1]) < 1e-5; }   // ellipsoid.h:46

// BinaryEllipsoidSystem (ellipsoid.h:303-364): f_AB = p / q, d f_AB / d lambda ~ h
struct Contact {
  M3 XA_m1, XB_m1;
  double p[5], q[4], h[7];
};
PK_FN double contact_f(const Contact &e, double l) {   // ellipsoid.h:365
  return (e.p[0] + l * (e.p[1] + l * (e.p[2] + l * (e.p[3] + l * e.p[4])))) / (e.q[0] + l * (e.q[1] + l * (e.q[2] + l * e.q[3])));
}
PK_FN double contact_fd(const double h[7], double l) {   // ellipsoid.h:368
  return h[0] + l * (h[1] + l * (h[2] + l * (h[3] + l * (h[4] + l * (h[5] + l * h[6])))));
}
PK_FN void contact_setup(Contact &e, const double ra[3], const Q4 &qa, const double rb[3], const Q4 &qb, const V3 &rij) {
  const M3 QA = quat_matrix(qa), QB = quat_matrix(qb);
  e.XA_m1 = shape_matrix(QA, ra[0] * ra[0], ra[1] * ra[1], ra[2] * ra[2]);
  e.XB_m1 = shape_matrix(QB, rb[0] * rb[0], rb[1] * rb[1], rb[2] * rb[2]);
  const M3 XB_12 = shape_matrix(QB, 1 / rb[0], 1 / rb[1], 1 / rb[2]);
  const M3 A = mmul(mmul(XB_12, e.XA_m1), XB_12);   // ellipsoid.h:321
  const V3 a = mvec(XB_12, rij);
  const double detA = det3(A);
  const M3 Z = adj3(A);
  M3 C1 = mscale(Z, -2), C2 = Z;   // ellipsoid.h:326-345
  C1.m[0][0] += A.m[1][1] + A.m[2][2];
  C1.m[1][1] += A.m[0][0] + A.m[2][2];
  C1.m[2][2] += A.m[1][1] + A.m[0][0];
  C1.m[0][1] -= A.m[1][0]; C1.m[0][2] -= A.m[2][0]; C1.m[1][0] -= A.m[0][1];
  C1.m[1][2] -= A.m[2][1]; C1.m[2][0] -= A.m[0][2]; C1.m[2][1] -= A.m[1][2];
  C2.m[0][0] -= A.m[1][1] + A.m[2][2] - 1;
  C2.m[1][1] -= A.m[0][0] + A.m[2][2] - 1;
  C2.m[2][2] -= A.m[1][1] + A.m[0][0] - 1;
  C2.m[0][1] += A.m[1][0]; C2.m[0][2] += A.m[2][0]; C2.m[1][0] += A.m[0][1];
  C2.m[1][2] += A.m[2][1]; C2.m[2][0] += A.m[0][2]; C2.m[2][1] += A.m[1][2];
  const double w0 = vmv3(Z, a), w1 = vmv3(C1, a), w2 = vmv3(C2, a);
  const double sa = A.m[0][0] + A.m[1][1] + A.m[2][2];
  const double sz = Z.m[0][0] + Z.m[1][1] + Z.m[2][2];
  double *p = e.p, *q = e.q, *h = e.h;
  if (fabs(detA) > 1e-5) {   // ellipsoid.h:351-357
    p[0] = 0; p[1] = w0; p[2] = w1 - w0; p[3] = w2 - w1; p[4] = -w2;
    q[0] = detA; q[1] = -3 * detA + sz; q[2] = 3 * detA + sa - 2 * sz; q[3] = 1 - detA - sa + sz;
    h[0] = q[0] * p[1];
    h[1] = 2 * q[0] * p[2];
    h[2] = 3 * q[0] * p[3] + q[1] * p[2] - q[2] * p[1];
    h[3] = 4 * q[0] * p[4] + 2 * q[1] * p[3] - 2 * q[3] * p[1];
    h[4] = 3 * q[1] * p[4] + q[2] * p[3] - q[3] * p[2];
    h[5] = 2 * q[2] * p[4];
    h[6] = q[3] * p[4];
  } else {   // a degenerate A_AB (a tiny A against a large B), ellipsoid.h:358-363
    p[0] = w0; p[1] = w1 - w0; p[2] = w2 - w1; p[3] = -w2; p[4] = 0;
    q[0] = sz; q[1] = sa - 2 * sz; q[2] = 1 - sa + sz; q[3] = 0;
    h[0] = q[0] * p[1];
    h[1] = 2 * q[0] * p[2];
    h[2] = 3 * q[0] * p[3] + q[1] * p[2] - q[2] * p[1];
    h[3] = 2 * q[1] * p[3];
    h[4] = q[2] * p[3];
    h[5] = 0; h[6] = 0;
  }
}

// zeroin(ell, 0, 1), packing.h:697-764 (Forsythe-Malcolm-Moler: bisection with linear or inverse quadratic interpolation).
// The reference loops for ever; here at most ROOT_CAP evaluations, after which *capped is set and the pair counts for nothing.
PK_FN double root_search(const double h[7], int *evals, bool *capped) {
  const double EPSILON = 1e-15;
  double a = 0., b = 1., c = a;
  double fa = contact_fd(h, a), fb = contact_fd(h, b), fc = fa;
  int n = 2;
  *capped = false;
  for (;;) {
    const double prev_step = b - a;
    if (fabs(fc) < fabs(fb)) { a = b; b = c; c = a; fa = fb; fb = fc; fc = fa; }
    const double tol_act = 2 * EPSILON * fabs(b) + 0.0 / 2;
    double new_step = (c - b) / 2;
    if (fabs(new_step) <= tol_act || fb == 0.) break;
    if (n >= ROOT_CAP) { *capped = true; break; }
    if (fabs(prev_step) >= tol_act && fabs(fa) > fabs(fb)) {
      const double cb = c - b;
      double p, q;
      if (a == c) {   // linear interpolation
        const double t1 = fb / fa;
        p = cb * t1;
        q = 1.0 - t1;
      } else {        // inverse quadratic
        q = fa / fc;
        const double t1 = fb / fc, t2 = fb / fa;
        p = t2 * (cb * q * (q - t1) - (b - a) * (t1 - 1.0));
        q = (q - 1.0) * (t1 - 1.0) * (t2 - 1.0);
      }
      if (p > 0.) q = -q; else p = -p;
      if (p < (0.75 * cb * q - fabs(tol_act * q) / 2) && p < fabs(prev_step * q / 2)) new_step = p / q;
    }
    if (fabs(new_step) < tol_act) new_step = new_step > 0. ? tol_act : -tol_act;
    a = b; fa = fb;
    b += new_step;
    fb = contact_fd(h, b);
    n++;
    if ((fb > 0 && fc > 0) || (fb < 0 && fc < 0)) { c = a; fc = fa; }
  }
  *evals = n;
  return b;
}

struct PairResult {
  int kind;       // 0: nothing (lambda < 1e-10 or the cap), 1: f_AB >= 1, 2: overlap
  int evals; bool capped;
  double lambda, fscl;   // fscl = 4 f_AB(lambda), the candidate for Dinner^2
  V3 n, f, tA, tB;       // f: B gains it, A loses it; tA, tB: the torque terms before their signs
};

// Packing::calc_forces(e, ei, ej), packing.h:108-144.  A is the particle of the higher index, rij = pos_B - pos_A.
PK_FN void pair_eval(PairResult &o, const double ra[3], const Q4 &qa, const double rb[3], const Q4 &qb, const V3 &rij, double Douter2, bool rotate) {
  const V3 z = {{0, 0, 0}};
  o.kind = 0; o.fscl = 0; o.n = z; o.f = z; o.tA = z; o.tB = z;
  Contact e;
  contact_setup(e, ra, qa, rb, qb, rij);
  const double lambda = root_search(e.h, &o.evals, &o.capped);
  o.lambda = lambda;
  if (o.capped || fabs(lambda) < 1e-10) return;   // :113-118
  o.fscl = 4 * contact_f(e, lambda);
  const double f_AB = o.fscl / Douter2;
  const M3 Y = madd(mscale(e.XB_m1, lambda), mscale(e.XA_m1, 1 - lambda));   // countY, ellipsoid.h:312
  o.n = mvec(mscale(adj3(Y), 1. / det3(Y)), rij);                              // count_n, :379; inverse, geometry.h:338
  o.kind = 1;
  if (f_AB >= 1) return;   // :122
  o.kind = 2;
  o.f = vmul(normalised(o.n), 1 - f_AB);   // :132
  if (!rotate) return;
  if (!sphere(ra)) o.tA = vmul(normalised(cross3(mvec(mscale(e.XA_m1, 1 - lambda), o.n), o.n)), 1 - f_AB);   // count_rac, :139
  if (!sphere(rb)) o.tB = vmul(normalised(cross3(mvec(mscale(e.XB_m1, -lambda), o.n), o.n)), 1 - f_AB);      // count_rbc, :141
}

// ---------------------------------------------------------------------------------------------------------------- device state
struct View {
  int N, K, ns, rotate;
  int grid[3], ncell_min;
  double box[3], half[3];
  double eps_scl, eps_rot, Rc_max, Diam_dens;
  Ctl *ctl;
  const int *spec;          // [N]
  const double *size;       // [ns][3]
  double *pos[3], *quat[4], *f[3], *fu[3];   // [N] each
  double *fnorm, *pmin;     // [N]: |f| before the move; the particle's smallest overlapping 4 f_AB
  int *pcell, *plow, *plen; // [N]: packed cell of the particle, low cell and length of its range per axis, bit 30 = all pairs
  int *cnt, *list;          // [N], [N][K]
  double *rec;              // [7][N K]: force[3], torque[3], Dinner^2 candidate of every list slot
  // walls (hc_packing_set_walls; DESIGN §6 "packing walls").  walls = 0: nothing below is read
  int walls, wrap[3], wd[3];   // wrap: the axis is periodic; wd: nodes of the wall field per axis
  double wsp, wmargin;         // node spacing and wall margin, in grid cells
  const double *snode;         // [wd0][wd1][wd2]: signed distance of a node to the wall surface, in node spacings
  double *wrec;                // [7][N]: the wall slot's force[3], torque[3] and Dinner^2 candidate
};

constexpr int ERR_ROOT_CAP = 1, ERR_WALL_NODE = 2;   // Ctl::error
constexpr double WALL_S_MIN = 1e-6;                   // the image pair is evaluated no closer to the surface than this (grid cells)

__device__ __forceinline__ bool halted(const Ctl *c) { return c->finished | c->error | c->grow; }

// ---------------------------------------------------------------------------------------------------------------- walls
// A node index along an axis: the floor modulo on a periodic axis, clamped to the field elsewhere.
PK_FN int wall_node(int i, int d, int wrap) {
  if (wrap) { i %= d; return i < 0 ? i + d : i; }
  return i < 0 ? 0 : (i > d - 1 ? d - 1 : i);
}
PK_FN double wall_floor(double u) {   // floor, kept where the conversion to int is defined
  double fl = floor(u);
  if (!(fl > -1e9)) fl = -1e9;
  if (fl > 1e9) fl = 1e9;
  return fl;
}
PK_FN double lerp(double a, double b, double t) { return a + t * (b - a); }

// s and n at x: the trilinear form of snode over the eight nodes around x and its analytic gradient.  Order: along z first
// (four edges), then y, then x; s = lerp(f0, f1, tx) wsp - wmargin.  false: the gradient's norm is below 1e-12.
PK_FN bool wall_sample(const View &v, const V3 &x, double *s, V3 *n) {
  int lo[3], hi[3]; double t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double u = x.v[k] / v.wsp, fl = wall_floor(u);
    t[k] = u - fl;
    lo[k] = wall_node((int)fl, v.wd[k], v.wrap[k]);
    hi[k] = wall_node((int)fl + 1, v.wd[k], v.wrap[k]);
  }
  const size_t sy = (size_t)v.wd[2], sx = sy * v.wd[1];
  const double c000 = v.snode[lo[0] * sx + lo[1] * sy + lo[2]], c001 = v.snode[lo[0] * sx + lo[1] * sy + hi[2]];
  const double c010 = v.snode[lo[0] * sx + hi[1] * sy + lo[2]], c011 = v.snode[lo[0] * sx + hi[1] * sy + hi[2]];
  const double c100 = v.snode[hi[0] * sx + lo[1] * sy + lo[2]], c101 = v.snode[hi[0] * sx + lo[1] * sy + hi[2]];
  const double c110 = v.snode[hi[0] * sx + hi[1] * sy + lo[2]], c111 = v.snode[hi[0] * sx + hi[1] * sy + hi[2]];
  const double e00 = lerp(c000, c001, t[2]), e01 = lerp(c010, c011, t[2]), e10 = lerp(c100, c101, t[2]), e11 = lerp(c110, c111, t[2]);
  const double f0 = lerp(e00, e01, t[1]), f1 = lerp(e10, e11, t[1]);
  *s = lerp(f0, f1, t[0]) * v.wsp - v.wmargin;
  V3 g;
  g.v[0] = f1 - f0;
  g.v[1] = lerp(e01 - e00, e11 - e10, t[0]);
  g.v[2] = lerp(lerp(c001 - c000, c011 - c010, t[1]), lerp(c101 - c100, c111 - c110, t[1]), t[0]);
  const double len = sqrt(dot3(g, g));
  if (!(len >= 1e-12)) return false;
  *n = vmul(g, 1 / len);
  return true;
}

// the node nearest to x is a wall node, or x lies off the field on an axis that does not wrap
PK_FN bool wall_hit(const View &v, const V3 &x) {
  int at[3];
  bool out = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double u = x.v[k] / v.wsp;
    if (!v.wrap[k] && !(u >= 0 && u <= v.wd[k] - 1)) out = true;
    at[k] = wall_node((int)wall_floor(u + 0.5), v.wd[k], v.wrap[k]);
  }
  return out || v.snode[((size_t)at[0] * v.wd[1] + at[1]) * v.wd[2] + at[2]] < 0;
}

// The wall as the particle's mirror image across the tangent plane at distance s along -n: same semi-axes, centre at
// x - 2 s n, orientation H R diag(1, 1, -1) with H = I - 2 n n^T.  As H = -Rot(n, pi) and diag(1, 1, -1) = -Rot(z, pi), the
// image's quaternion is the product (0, z) q (0, n) in quat_mul's order: no branch, the sign is the product's.
PK_FN void wall_eval(PairResult &o, const double r[3], const Q4 &q, double s, const V3 &n, double Douter2, bool rotate) {
  const double se = s > WALL_S_MIN ? s : WALL_S_MIN;
  Q4 qz; qz.s = 0; qz.p.v[0] = 0; qz.p.v[1] = 0; qz.p.v[2] = 1;
  Q4 qn; qn.s = 0; qn.p = n;
  const Q4 qi = quat_mul(quat_mul(qz, q), qn);
  pair_eval(o, r, q, r, qi, vmul(n, -2 * se), Douter2, rotate);
  // a principal axis along n: X n is parallel to n, the torque's direction is 0/0 in pair_eval, and by symmetry there is none
  if (o.tA.v[0] != o.tA.v[0] || o.tA.v[1] != o.tA.v[1] || o.tA.v[2] != o.tA.v[2]) { o.tA.v[0] = 0; o.tA.v[1] = 0; o.tA.v[2] = 0; }
}

// calc_motion (packing.h:399-428) and, by the first thread, Douter -= Relax (iterate, :347-348): nothing here reads Douter.
// WALLS: only periodic axes wrap; a centre that lands on a wall node or off the field sets the error flag.
template <bool WALLS>
__global__ __launch_bounds__(256) void pk_motion(View v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (halted(v.ctl)) return;
  if (i == 0) { const double D = v.ctl->Douter - v.ctl->Relax; v.ctl->Douter = D; v.ctl->Douter2 = D * D; }
  if (i >= v.N) return;
  V3 f, fu;
#pragma unroll
  for (int k = 0; k < 3; k++) { f.v[k] = v.f[k][i]; fu.v[k] = v.fu[k][i]; }
  v.fnorm[i] = sqrt(dot3(f, f));   // :408
  V3 xn;
#pragma unroll
  for (int k = 0; k < 3; k++) {    // :410-412, vector3::pbc (geometry.h:104-112)
    double x = v.pos[k][i] + f.v[k] * v.eps_scl;
    if (!WALLS || v.wrap[k]) { if (x < 0) x += v.box[k]; else if (x > v.box[k]) x -= v.box[k]; }
    v.pos[k][i] = x;
    xn.v[k] = x;
  }
  if (WALLS && wall_hit(v, xn)) atomicMax(&v.ctl->error, ERR_WALL_NODE);
  if (!v.rotate || sphere(v.size + 3 * v.spec[i])) return;   // :415-417
  const double len = v.eps_rot * sqrt(dot3(fu, fu));
  const double cp = 1 / sqrt(1 + len * len);
  const double sp = len * cp;
  const double cp2 = sqrt(0.5 * (1 + cp));
  const double sp2 = 0.5 * sp / cp2;
  Q4 t; t.s = v.quat[0][i];
#pragma unroll
  for (int k = 0; k < 3; k++) t.p.v[k] = v.quat[1 + k][i];
  const Q4 r = quat_mul(t, quat_unit(cp2, vmul(fu, sp2)));   // :423-424
  v.quat[0][i] = r.s;
#pragma unroll
  for (int k = 0; k < 3; k++) v.quat[1 + k][i] = r.p.v[k];
}

// The particle's own grid cell and, as A, its mode and cell range (packing.h:387-395, :438-443).  10 bits per axis.
__global__ __launch_bounds__(256) void pk_bin(View v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (halted(v.ctl) || i >= v.N) return;
  const double Rcut = 0.55 * v.ctl->Douter * (v.size[3 * v.spec[i]] + v.Rc_max);
  const bool part = (int)(2.0 * Rcut) < v.ncell_min - 1;
  int cell = 0, low = 0, len = 0;
  bool in_grid = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double x = v.pos[k][i];
    const int c = (int)x;   // x == box is possible (pbc keeps it); the reference would index past its cell array there
    if (c < 0 || c >= v.grid[k]) in_grid = false;
    const int lo = (int)(x + v.grid[k] - Rcut), hi = (int)(x + v.grid[k] + Rcut);
    int span = hi - lo;
    if (span > v.grid[k] - 1) span = v.grid[k] - 1;   // cannot happen in this mode ((int)(2 Rcut) + 1 <= N - 1); keeps the fields in range
    if (span < 0) span = 0;
    const int lom = ((lo % v.grid[k]) + v.grid[k]) % v.grid[k];
    cell |= (c & 1023) << (10 * k); low |= lom << (10 * k); len |= span << (10 * k);
  }
  v.pcell[i] = in_grid ? cell : -1;
  v.plow[i] = low;
  v.plen[i] = len | (part ? 0 : 1 << 30);
}

__device__ __forceinline__ bool partner(const View &v, int cellB, int lowA, int lenA) {
  if (lenA & (1 << 30)) return true;   // force_all: every B < A
  if (cellB < 0) return false;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int d = ((cellB >> (10 * k)) & 1023) - ((lowA >> (10 * k)) & 1023);
    if (d < 0) d += v.grid[k];
    in = in && d <= ((lenA >> (10 * k)) & 1023);
  }
  return in;
}

// One wave per particle i: its partners j in ascending order.  With A = max(i, j), B = min(i, j) the pair is active when A
// runs on all pairs or B's cell lies in A's range (force_part keeps no distance test, packing.h:446-462).
__global__ __launch_bounds__(256) void pk_list(View v) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (halted(v.ctl) || i >= v.N) return;
  const int cell_i = v.pcell[i], low_i = v.plow[i], len_i = v.plen[i];
  int total = 0;
  for (int base = 0; base < v.N; base += 64) {
    const int j = base + lane;
    bool act = false;
    if (j < v.N && j != i) act = j < i ? partner(v, v.pcell[j], low_i, len_i) : partner(v, cell_i, v.plow[j], v.plen[j]);
    const unsigned long long m = __ballot(act);
    const int at = total + __popcll(m & ((1ull << lane) - 1ull));
    if (act && at < v.K) v.list[(size_t)i * v.K + at] = j;
    total += __popcll(m);
  }
  if (lane == 0) {
    v.cnt[i] = total < v.K ? total : v.K;
    atomicMax(&v.ctl->maxcount, total);
    if (total > v.K) atomicMax(&v.ctl->grow, 1);   // the list is short: everything after this kernel is skipped until it has grown
  }
}

__device__ __forceinline__ void load_particle(const View &v, int i, double r[3], Q4 &q, V3 &x) {
  const int s = v.spec[i];
#pragma unroll
  for (int k = 0; k < 3; k++) { r[k] = v.size[3 * s + k]; x.v[k] = v.pos[k][i]; q.p.v[k] = v.quat[1 + k][i]; }
  q.s = v.quat[0][i];
}

// One thread per list slot: the pair (A, B) of particle i and its partner, and i's own share of it.
// WALLS: the minimum image is taken on periodic axes only.
template <bool WALLS>
__global__ __launch_bounds__(256) void pk_pair(View v) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (halted(v.ctl)) return;
  const int i = (int)(t / v.K), s = (int)(t % v.K);
  if (i >= v.N || s >= v.cnt[i]) return;
  const int j = v.list[t];
  const int A = i > j ? i : j, B = i > j ? j : i;
  double ra[3], rb[3]; Q4 qa, qb; V3 xa, xb, rij;
  load_particle(v, A, ra, qa, xa);
  load_particle(v, B, rb, qb, xb);
#pragma unroll
  for (int k = 0; k < 3; k++) {   // rij = pos_B - pos_A, then pbc_diff (packing.h:483-484, geometry.h:113-121), on both paths
    double d = xb.v[k] - xa.v[k];
    if (!WALLS || v.wrap[k]) { if (d < -v.half[k]) d += v.box[k]; else if (d > v.half[k]) d -= v.box[k]; }
    rij.v[k] = d;
  }
  const double Douter2 = v.ctl->Douter2;
  PairResult o;
  pair_eval(o, ra, qa, rb, qb, rij, Douter2, v.rotate != 0);
  atomicMax(&v.ctl->maxeval, o.evals);
  if (o.capped) atomicMax(&v.ctl->error, ERR_ROOT_CAP);
  const size_t stride = (size_t)v.N * v.K;
  const bool isA = i == A;
  const V3 tq = isA ? o.tA : o.tB;
#pragma unroll
  for (int k = 0; k < 3; k++) {   // A: f -= f, fu -= t; B: f += f, fu += t (:133-134, :140-142)
    v.rec[k * stride + t] = isA ? -o.f.v[k] : o.f.v[k];
    v.rec[(3 + k) * stride + t] = isA ? -tq.v[k] : tq.v[k];
  }
  v.rec[6 * stride + t] = o.kind == 2 ? o.fscl : Douter2;   // :131, overlapping pairs only
}

// The wall slot of particle i, one thread each: while s < 0.55 Douter (largest axis), pk_bin's cut-off for a pair of two such
// particles halved, i takes the A side of the pair with its mirror image.  Without the slot (beyond the cut-off, or no
// gradient) the record is what a pair that does not overlap leaves: zero force and torque, Douter^2 as candidate.
__global__ __launch_bounds__(256) void pk_wall(View v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (halted(v.ctl) || i >= v.N) return;
  double r[3]; Q4 q; V3 x;
  load_particle(v, i, r, q, x);
  double amax = r[0];
  if (r[1] > amax) amax = r[1];
  if (r[2] > amax) amax = r[2];
  const double Douter2 = v.ctl->Douter2;
  const double cut = 0.55 * v.ctl->Douter * amax;
  double rec[7] = {0, 0, 0, 0, 0, 0, Douter2};
  double s; V3 n;
  if (wall_sample(v, x, &s, &n) && s < cut) {
    PairResult o;
    wall_eval(o, r, q, s, n, Douter2, v.rotate != 0);
    atomicMax(&v.ctl->maxeval, o.evals);
    if (o.capped) atomicMax(&v.ctl->error, ERR_ROOT_CAP);
#pragma unroll
    for (int k = 0; k < 3; k++) { rec[k] = -o.f.v[k]; rec[3 + k] = -o.tA.v[k]; }
    if (o.kind == 2) rec[6] = o.fscl;
  }
#pragma unroll
  for (int k = 0; k < 7; k++) v.wrec[(size_t)k * v.N + i] = rec[k];
}

// A particle's force and torque: its slots added in list order, which is ascending partner index; WALLS: then the wall slot.
template <bool WALLS>
__global__ __launch_bounds__(256) void pk_sum(View v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (halted(v.ctl) || i >= v.N) return;
  const size_t stride = (size_t)v.N * v.K, at = (size_t)i * v.K;
  double a[6] = {0, 0, 0, 0, 0, 0}, dmin = v.ctl->Douter2;   // :372
  const int n = v.cnt[i];
  for (int s = 0; s < n; s++) {
#pragma unroll
    for (int k = 0; k < 6; k++) a[k] += v.rec[k * stride + at + s];
    const double d = v.rec[6 * stride + at + s];
    if (d < dmin) dmin = d;
  }
  if (WALLS) {
#pragma unroll
    for (int k = 0; k < 6; k++) a[k] += v.wrec[(size_t)k * v.N + i];
    const double d = v.wrec[(size_t)6 * v.N + i];
    if (d < dmin) dmin = d;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { v.f[k][i] = a[k]; v.fu[k][i] = a[3 + k]; }
  v.pmin[i] = dmin;
}

__device__ const double PK_POW10_NEG[NFIG] = {1e-0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12, 1e-13, 1e-14, 1e-15};

// One workgroup: Dinner (the minimum) and Force_step (a sum in a fixed order: each thread strides, then a fixed tree) over the
// particles; its first thread then advances the control scalars as the tail of iterate() does (packing.h:351-367).
// first = 1: the calc_forces before the first iteration (execute, :179-182), which only sets Dinner and Pactual.
__global__ __launch_bounds__(256) void pk_control(View v, int first) {
  __shared__ double s_sum[256], s_min[256];
  Ctl *c = v.ctl;
  if (halted(c)) return;   // uniform: nothing in this kernel has written c yet
  double sum = 0, mn = c->Douter2;
  for (int i = threadIdx.x; i < v.N; i += 256) {
    if (!first) sum += v.fnorm[i];
    const double d = v.pmin[i];
    if (d < mn) mn = d;
  }
  s_sum[threadIdx.x] = sum; s_min[threadIdx.x] = mn;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
      if (s_min[threadIdx.x + off] < s_min[threadIdx.x]) s_min[threadIdx.x] = s_min[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double Dinner = sqrt(s_min[0]);   // :396
  c->Dinner = Dinner;
  c->Pactual = Dinner * Dinner * Dinner / v.Diam_dens;
  if (first) return;
  const double Douter = c->Douter;
  c->DensityNominal = Douter * Douter * Douter / v.Diam_dens;
  c->Force_step = s_sum[0] / v.N;   // :427
  c->steps++;
  if (c->Force_step < 1e-15) { c->finished = 1; return; }   // :355-360
  if (c->doExit) return;
  // iprec = (int)(-log10(d)) >= Nsf is d > 0 && d <= 10^-Nsf in exact arithmetic (:363-364); no library call on the device
  const double d = c->DensityNominal - c->Pactual;
  if (d > 0 && d <= PK_POW10_NEG[c->Nsf]) {
    c->Relax *= 0.5;
    if (++c->Nsf >= NFIG) c->doExit = 1;
  }
}

// hc_packing_pairs: the same pair_eval on caller-given pairs
__global__ __launch_bounds__(256) void pk_probe(int n, const double *in /*[n][21]*/, int rotate, double *out /*[n][17]*/, int *iout /*[n][3]*/) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const double *x = in + 21 * (size_t)t;
  double ra[3], rb[3]; V3 pa, pb, rij;
#pragma unroll
  for (int k = 0; k < 3; k++) { ra[k] = x[k]; pa.v[k] = x[4 + k]; rb[k] = x[7 + k]; pb.v[k] = x[11 + k]; rij.v[k] = x[14 + k]; }
  const Q4 qa = quat_make(x[3], pa), qb = quat_make(x[10], pb);
  PairResult o;
  pair_eval(o, ra, qa, rb, qb, rij, x[17], rotate != 0);
  double *y = out + 17 * (size_t)t;
  y[0] = o.lambda; y[1] = o.fscl;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    y[2 + k] = o.n.v[k];
    y[5 + k] = 0.0 - o.f.v[k];
    y[8 + k] = 0.0 - o.tA.v[k];
    y[11 + k] = 0.0 + o.f.v[k];
    y[14 + k] = 0.0 + o.tB.v[k];
  }
  iout[3 * t] = o.kind; iout[3 * t + 1] = o.evals; iout[3 * t + 2] = o.capped ? 1 : 0;
}

// hc_packing_walls: the same wall_eval on caller-given particles, distances and normals
__global__ __launch_bounds__(256) void pk_wall_probe(int n, const double *in /*[n][12]*/, int rotate, double *out /*[n][7]*/, int *iout /*[n][3]*/) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const double *x = in + 12 * (size_t)t;
  double r[3]; V3 p, nv;
#pragma unroll
  for (int k = 0; k < 3; k++) { r[k] = x[k]; p.v[k] = x[4 + k]; nv.v[k] = x[8 + k]; }
  const Q4 q = quat_make(x[3], p);
  PairResult o;
  wall_eval(o, r, q, x[7], nv, x[11], rotate != 0);
  double *y = out + 7 * (size_t)t;
#pragma unroll
  for (int k = 0; k < 3; k++) { y[k] = 0.0 - o.f.v[k]; y[3 + k] = 0.0 - o.tA.v[k]; }
  y[6] = o.kind == 2 ? o.fscl : x[11];
  iout[3 * t] = o.kind; iout[3 * t + 1] = o.evals; iout[3 * t + 2] = o.capped ? 1 : 0;
}

// The wall's distance field: exact squared Euclidean distance in node spacings from every node to the nearest wall node,
// truncated at R, as three separable passes min_k g[k] + (k - j)^2 on integers (z, then y, then x).  One thread per node
// with z fastest, so that the lanes of a wave read consecutive z in every pass.  Integer minima: no order dependence.
constexpr int EDT_FAR = 1 << 29;
__global__ __launch_bounds__(256) void pk_edt_init(size_t n, const unsigned char *mask, int *g) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) g[t] = mask[t] ? 0 : EDT_FAR;
}
__global__ __launch_bounds__(256) void pk_edt_pass(size_t n, const int *in, int *out, int d0, int d1, int d2, int axis, int wrap, int R) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int z = (int)(t % d2), y = (int)((t / d2) % d1), x = (int)(t / ((size_t)d2 * d1));
  const int j = axis == 0 ? x : (axis == 1 ? y : z), d = axis == 0 ? d0 : (axis == 1 ? d1 : d2);
  const size_t stride = axis == 0 ? (size_t)d1 * d2 : (axis == 1 ? (size_t)d2 : 1);
  const size_t base = t - (size_t)j * stride;
  int best = EDT_FAR;
  for (int o = -R; o <= R; o++) {
    int k = j + o;
    if (wrap) { k %= d; if (k < 0) k += d; }
    else if (k < 0 || k >= d) continue;
    const int g = in[base + (size_t)k * stride];
    if (g < EDT_FAR && g + o * o < best) best = g + o * o;
  }
  out[t] = best;
}
__global__ __launch_bounds__(256) void pk_edt_finish(size_t n, const int *g, int R, double *snode) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int d2 = g[t] < R * R ? g[t] : R * R;
  snode[t] = sqrt((double)d2) - 0.5;   // the surface lies halfway to the wall node; a wall node gets -0.5
}

}  // namespace

struct hc_packing {
  View v;
  hc::DevBuf<Ctl> ctl;
  hc::DevBuf<int> spec, ints, list;   // ints: pcell, plow, plen, cnt
  hc::DevBuf<double> size, part, rec; // part: pos, quat, f, fu, fnorm, pmin = 15 arrays of N
  bool resume = false;                // an iteration moved the particles and then found the lists too short
  size_t max_slots;
  hc::DevBuf<double> snode, wrec;     // walls: the distance field and the wall slots' records
  bool started = false;               // a run has queued iterations: too late for hc_packing_set_walls
  int wall_R = 0;                     // truncation of the distance field, in nodes
};

namespace {

constexpr size_t PK_MAX_SLOTS = (size_t)1 << 28;   // list slots; 7 doubles of records each = 14 GiB at the limit

int pk_reserve_pairs(hc_packing *P, int K) {
  const size_t slots = (size_t)P->v.N * K;
  if (slots > PK_MAX_SLOTS) { hc::set_error("hc_packing: the pair storage would exceed 2^28 slots (a grid this coarse puts too many particles in range of each other)"); return HC_ERR_ARG; }
  int rc;
  if ((rc = P->list.reserve(slots)) != HC_OK || (rc = P->rec.reserve(7 * slots)) != HC_OK) return rc;
  P->v.K = K; P->v.list = P->list; P->v.rec = P->rec;
  return HC_OK;
}

// bin, list, pair, sum, control: calc_forces and the tail of an iteration
void pk_queue_forces(hc_packing *P, int first) {
  const View &v = P->v;
  const unsigned nb = (unsigned)((v.N + 255) / 256);
  hipLaunchKernelGGL(pk_bin, dim3(nb), dim3(256), 0, hc::stream(), v);
  hipLaunchKernelGGL(pk_list, dim3((unsigned)((v.N + 3) / 4)), dim3(256), 0, hc::stream(), v);
  const dim3 slots((unsigned)(((size_t)v.N * v.K + 255) / 256));
  if (v.walls) {
    hipLaunchKernelGGL(pk_pair<true>, slots, dim3(256), 0, hc::stream(), v);
    hipLaunchKernelGGL(pk_wall, dim3(nb), dim3(256), 0, hc::stream(), v);
    hipLaunchKernelGGL(pk_sum<true>, dim3(nb), dim3(256), 0, hc::stream(), v);
  } else {
    hipLaunchKernelGGL(pk_pair<false>, slots, dim3(256), 0, hc::stream(), v);
    hipLaunchKernelGGL(pk_sum<false>, dim3(nb), dim3(256), 0, hc::stream(), v);
  }
  hipLaunchKernelGGL(pk_control, dim3(1), dim3(256), 0, hc::stream(), v, first);
}

int pk_read_ctl(hc_packing *P, Ctl *c) {
  HC_HIP(hipMemcpyAsync(c, P->ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

// after a wait that found grow set: larger lists, flag cleared
int pk_grow(hc_packing *P, const Ctl &c) {
  int K = c.maxcount + c.maxcount / 4 + 16;
  if (K > P->v.N - 1) K = P->v.N - 1;
  if (K < 1) K = 1;
  int rc = pk_reserve_pairs(P, K);
  if (rc != HC_OK) return rc;
  HC_HIP(hipMemsetAsync(&P->ctl.p->grow, 0, sizeof(int), hc::stream()));
  return HC_OK;
}

bool all_finite(const double *x, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(x[i])) return false; return true; }

}  // namespace

extern "C" {

int hc_packing_create(hc_packing **out, const int grid[3], int n_species, const double *sizes, const int *counts, const double *pos,
                      const double *quat, double nominal_density, int rotate, int ntau, double epsilon) {
  HC_REQUIRE(out && grid && sizes && counts && pos, "hc_packing_create: null pointer");
  *out = nullptr;
  HC_REQUIRE(n_species >= 1, "hc_packing_create: no species");
  for (int k = 0; k < 3; k++) HC_REQUIRE(grid[k] >= 1 && grid[k] <= 1023, "hc_packing_create: grid cells per axis must be 1..1023");
  long total = 0;
  for (int s = 0; s < n_species; s++) { HC_REQUIRE(counts[s] >= 0, "hc_packing_create: negative species count"); total += counts[s]; }
  HC_REQUIRE(total >= 1, "hc_packing_create: no particles (every species count is zero)");
  HC_REQUIRE(total < (1L << 30), "hc_packing_create: too many particles");
  const int N = (int)total;
  HC_REQUIRE(all_finite(sizes, 3 * (size_t)n_species), "hc_packing_create: non-finite species size");
  for (int s = 0; s < 3 * n_species; s++) HC_REQUIRE(sizes[s] > 0, "hc_packing_create: species sizes must be positive");
  HC_REQUIRE(all_finite(pos, 3 * (size_t)N), "hc_packing_create: non-finite position");
  HC_REQUIRE(!quat || all_finite(quat, 4 * (size_t)N), "hc_packing_create: non-finite quaternion");
  HC_REQUIRE(std::isfinite(nominal_density) && nominal_density > 0, "hc_packing_create: nominal density must be positive and finite");
  HC_REQUIRE(std::isfinite(epsilon), "hc_packing_create: non-finite epsilon");
  for (int i = 0; i < N; i++)
    for (int k = 0; k < 3; k++) HC_REQUIRE(pos[3 * i + k] >= 0 && pos[3 * i + k] <= grid[k], "hc_packing_create: position outside the box");
  if (ntau <= 0) ntau = 102400;        // packing.h:225
  if (!(epsilon > 0)) epsilon = 0.1;   // :202

  hc_packing *P = new hc_packing;
  View &v = P->v;
  v.N = N; v.ns = n_species; v.rotate = rotate ? 1 : 0;
  v.walls = 0; v.wsp = 1; v.wmargin = 0; v.snode = nullptr; v.wrec = nullptr;
  for (int k = 0; k < 3; k++) { v.wrap[k] = 1; v.wd[k] = 0; }
  // Packing::init, packing.h:268-289
  const int No_cells = grid[0] * grid[1] * grid[2];
  v.ncell_min = grid[0] < grid[1] ? grid[0] : grid[1];
  if (grid[2] < v.ncell_min) v.ncell_min = grid[2];
  for (int k = 0; k < 3; k++) { v.grid[k] = grid[k]; v.box[k] = grid[k]; v.half[k] = 0.5 * v.box[k]; }
  double Diam_dens = No_cells / (3.141592653589793 / 6.);
  double corr = 0;
  v.Rc_max = 0;
  for (int s = 0; s < n_species; s++) { corr += counts[s]; if (sizes[3 * s] > v.Rc_max) v.Rc_max = sizes[3 * s]; }
  Diam_dens /= corr;
  v.Diam_dens = Diam_dens;
  Ctl c{};
  c.DensityNominal = nominal_density;
  const double Douter0 = std::pow(Diam_dens * nominal_density, 1. / 3.);
  c.Douter = Douter0;
  c.Relax = 0.5 * c.Douter / ntau;
  c.Douter2 = c.Douter * c.Douter;
  c.Nsf = 1;
  const double alpha = sizes[0];
  v.eps_rot = 50. / (alpha * alpha * alpha);   // :288-289 (initBlood's 3.0 is above .1)
  v.eps_scl = epsilon * Douter0;                // :402

  // list length: twice the mean number of particles in the largest cell range at the first diameter, plus slack; all of them
  // where a species still runs on all pairs
  const double Rcut0 = 0.55 * Douter0 * (v.Rc_max + v.Rc_max);
  int K;
  if (!((int)(2.0 * Rcut0) < v.ncell_min - 1)) K = N - 1;
  else {
    double cells = 1;
    for (int k = 0; k < 3; k++) { const double w = 2 * Rcut0 + 2; cells *= w < grid[k] ? w : grid[k]; }
    const double mean = cells * N / No_cells;
    K = (int)(2 * mean) + 64;
    if (K > N - 1) K = N - 1;
  }
  if (K < 1) K = 1;

  auto fail = [&](int rc) { delete P; return rc; };
  int rc;
  if ((rc = P->ctl.reserve(1)) != HC_OK || (rc = P->spec.reserve(N)) != HC_OK || (rc = P->ints.reserve(4 * (size_t)N)) != HC_OK ||
      (rc = P->size.reserve(3 * (size_t)n_species)) != HC_OK || (rc = P->part.reserve(15 * (size_t)N)) != HC_OK || (rc = pk_reserve_pairs(P, K)) != HC_OK)
    return fail(rc);
  v.ctl = P->ctl; v.spec = P->spec; v.size = P->size;
  double *d = P->part;
  for (int k = 0; k < 3; k++) v.pos[k] = d + (size_t)k * N;
  for (int k = 0; k < 4; k++) v.quat[k] = d + (size_t)(3 + k) * N;
  for (int k = 0; k < 3; k++) { v.f[k] = d + (size_t)(7 + k) * N; v.fu[k] = d + (size_t)(10 + k) * N; }
  v.fnorm = d + (size_t)13 * N; v.pmin = d + (size_t)14 * N;
  v.pcell = P->ints; v.plow = P->ints + N; v.plen = P->ints + 2 * (size_t)N; v.cnt = P->ints + 3 * (size_t)N;

  std::vector<int> spec(N);
  std::vector<double> h(15 * (size_t)N, 0.0);
  int at = 0;
  for (int s = 0; s < n_species; s++) for (int q = 0; q < counts[s]; q++) spec[at++] = s;
  for (int i = 0; i < N; i++) {
    for (int k = 0; k < 3; k++) h[(size_t)k * N + i] = pos[3 * i + k];
    for (int k = 0; k < 4; k++) h[(size_t)(3 + k) * N + i] = quat ? quat[4 * i + k] : (k == 0 ? 1.0 : 0.0);   // identity, ellipsoid.h:70
  }
  hipError_t e = hipMemcpy(P->spec, spec.data(), N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(P->size, sizes, 3 * (size_t)n_species * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(P->part, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(P->ctl, &c, sizeof c, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(hc::hip_fail(e, "hipMemcpy", __FILE__, __LINE__));

  // the calc_forces before the first iteration (execute, :179-182); the lists may grow here as often as needed
  for (int attempt = 0;; attempt++) {
    pk_queue_forces(P, 1);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(hc::hip_fail(e, "packing kernels", __FILE__, __LINE__));
    if ((rc = pk_read_ctl(P, &c)) != HC_OK) return fail(rc);
    if (c.error) { hc::set_error("hc_packing_create: a pair's root search did not end within 256 evaluations"); return fail(HC_ERR_STATE); }
    if (!c.grow) break;
    if (attempt >= 4) { hc::set_error("hc_packing_create: the pair lists did not settle"); return fail(HC_ERR_STATE); }
    if ((rc = pk_grow(P, c)) != HC_OK) return fail(rc);
  }
  *out = P;
  return HC_OK;
}

int hc_packing_run(hc_packing *P, int max_steps, double status[12]) {
  HC_REQUIRE(P && status, "hc_packing_run: null pointer");
  HC_REQUIRE(max_steps >= 0, "hc_packing_run: max_steps < 0");
  const View &v = P->v;
  const unsigned nb = (unsigned)((v.N + 255) / 256);
  if (max_steps > 0) P->started = true;
  for (int s = 0; s < max_steps; s++) {
    if (!P->resume) {
      if (v.walls) hipLaunchKernelGGL(pk_motion<true>, dim3(nb), dim3(256), 0, hc::stream(), v);
      else hipLaunchKernelGGL(pk_motion<false>, dim3(nb), dim3(256), 0, hc::stream(), v);
    }
    P->resume = false;
    pk_queue_forces(P, 0);
  }
  HC_HIP(hipGetLastError());
  Ctl c;
  int rc = pk_read_ctl(P, &c);
  if (rc != HC_OK) return rc;
  status[0] = c.steps; status[1] = c.finished; status[2] = c.Douter; status[3] = c.Dinner; status[4] = c.Pactual; status[5] = c.DensityNominal;
  status[6] = c.Force_step; status[7] = c.Relax; status[8] = c.Nsf; status[9] = c.error; status[10] = c.maxeval; status[11] = c.grow;
  if (c.error == ERR_WALL_NODE) { hc::set_error("hc_packing_run: a particle's centre reached a wall node or left the wall field"); return HC_ERR_STATE; }
  if (c.error) { hc::set_error("hc_packing_run: a pair's root search did not end within 256 evaluations (non-finite state?)"); return HC_ERR_STATE; }
  if (c.grow) {   // between runs: the interrupted iteration has moved and has no forces yet; the next run starts with them
    if ((rc = pk_grow(P, c)) != HC_OK) return rc;
    P->resume = true;
  }
  return HC_OK;
}

int hc_packing_count(const hc_packing *P, int *n_particles, int *list_capacity) {
  HC_REQUIRE(P, "hc_packing_count: null pointer");
  if (n_particles) *n_particles = P->v.N;
  if (list_capacity) *list_capacity = P->v.K;
  return HC_OK;
}

int hc_packing_state(hc_packing *P, double *pos, double *quat, double *force, double *torque) {
  HC_REQUIRE(P, "hc_packing_state: null pointer");
  const int N = P->v.N;
  std::vector<double> h(13 * (size_t)N);
  HC_HIP(hipMemcpyAsync(h.data(), P->part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  for (int i = 0; i < N; i++) {
    for (int k = 0; k < 3; k++) {
      if (pos) pos[3 * i + k] = h[(size_t)k * N + i];
      if (force) force[3 * i + k] = h[(size_t)(7 + k) * N + i];
      if (torque) torque[3 * i + k] = h[(size_t)(10 + k) * N + i];
    }
    if (quat) for (int k = 0; k < 4; k++) quat[4 * i + k] = h[(size_t)(3 + k) * N + i];
  }
  return HC_OK;
}

int hc_packing_pairs(int n, const double *size_a, const double *quat_a, const double *size_b, const double *quat_b, const double *rij,
                     const double *douter2, int rotate, double *lambda, double *f_ab_scl, double *nvec, double *f_a, double *t_a,
                     double *f_b, double *t_b, int *evals, int *kind) {
  HC_REQUIRE(n >= 0, "hc_packing_pairs: n < 0");
  if (n == 0) return HC_OK;
  HC_REQUIRE(size_a && quat_a && size_b && quat_b && rij && douter2 && lambda && f_ab_scl && nvec && f_a && t_a && f_b && t_b && evals && kind,
             "hc_packing_pairs: null pointer");
  std::vector<double> in(21 * (size_t)n), outv(17 * (size_t)n);
  std::vector<int> iout(3 * (size_t)n);
  for (int t = 0; t < n; t++) {
    double *x = &in[21 * (size_t)t];
    for (int k = 0; k < 3; k++) { x[k] = size_a[3 * t + k]; x[7 + k] = size_b[3 * t + k]; x[14 + k] = rij[3 * t + k]; }
    for (int k = 0; k < 4; k++) { x[3 + k] = quat_a[4 * t + k]; x[10 + k] = quat_b[4 * t + k]; }
    x[17] = douter2[t]; x[18] = x[19] = x[20] = 0;
  }
  HC_REQUIRE(all_finite(in.data(), in.size()), "hc_packing_pairs: non-finite input");
  hc::DevBuf<double> din, dout; hc::DevBuf<int> diout;
  int rc;
  if ((rc = din.reserve(in.size())) != HC_OK || (rc = dout.reserve(outv.size())) != HC_OK || (rc = diout.reserve(iout.size())) != HC_OK) return rc;
  HC_HIP(hipMemcpyAsync(din.p, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice, hc::stream()));
  hipLaunchKernelGGL(pk_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), n, (const double *)din.p, rotate, dout.p, diout.p);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(outv.data(), dout.p, outv.size() * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipMemcpyAsync(iout.data(), diout.p, iout.size() * sizeof(int), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  for (int t = 0; t < n; t++) {
    const double *y = &outv[17 * (size_t)t];
    lambda[t] = y[0]; f_ab_scl[t] = y[1];
    for (int k = 0; k < 3; k++) { nvec[3 * t + k] = y[2 + k]; f_a[3 * t + k] = y[5 + k]; t_a[3 * t + k] = y[8 + k]; f_b[3 * t + k] = y[11 + k]; t_b[3 * t + k] = y[14 + k]; }
    evals[t] = iout[3 * t + 1];
    kind[t] = iout[3 * t + 2] ? -1 : iout[3 * t];
  }
  return HC_OK;
}

int hc_packing_reserve_lists(hc_packing *P, int capacity) {
  HC_REQUIRE(P, "hc_packing_reserve_lists: null pointer");
  HC_REQUIRE(capacity >= 1, "hc_packing_reserve_lists: the capacity must be at least 1");
  if (capacity > P->v.N - 1) capacity = P->v.N > 1 ? P->v.N - 1 : 1;
  return pk_reserve_pairs(P, capacity);   // the lists are rebuilt by every force evaluation; one that does not fit grows them
}

int hc_packing_set_walls(hc_packing *P, const unsigned char *mask, const int dims[3], double spacing, const int periodic[3], double wall_margin) {
  HC_REQUIRE(P && mask && dims && periodic, "hc_packing_set_walls: null pointer");
  HC_REQUIRE(!P->started, "hc_packing_set_walls: the packing has run; walls are set before the first hc_packing_run");
  HC_REQUIRE(!P->v.walls, "hc_packing_set_walls: walls are already set");
  HC_REQUIRE(std::isfinite(spacing) && spacing > 0, "hc_packing_set_walls: the spacing must be positive and finite");
  HC_REQUIRE(std::isfinite(wall_margin) && wall_margin >= 0, "hc_packing_set_walls: the wall margin must be finite and not negative");
  View &v = P->v;
  size_t n = 1;
  for (int k = 0; k < 3; k++) {
    HC_REQUIRE(dims[k] >= 2 && dims[k] <= 4096, "hc_packing_set_walls: mask nodes per axis must be 2..4096");
    n *= (size_t)dims[k];
    if (periodic[k])
      HC_REQUIRE(std::fabs(dims[k] * spacing - v.box[k]) <= 1e-9 * v.box[k],
                 "hc_packing_set_walls: the mask and the box disagree: on a periodic axis nodes x spacing must equal the box");
    else
      HC_REQUIRE((dims[k] - 1) * spacing <= v.box[k] * (1 + 1e-9),
                 "hc_packing_set_walls: the mask and the box disagree: the mask is longer than the box");
  }
  HC_REQUIRE(n < ((size_t)1 << 31), "hc_packing_set_walls: too many mask nodes");
  const size_t sy = (size_t)dims[2], sx = sy * dims[1];
  for (int k = 0; k < 3; k++) {
    if (periodic[k]) continue;
    const int a = (k + 1) % 3, b = (k + 2) % 3;
    const size_t st[3] = {sx, sy, 1};
    bool closed = true;
    for (int i = 0; i < dims[a] && closed; i++)
      for (int j = 0; j < dims[b]; j++) {
        const size_t at = i * st[a] + j * st[b];
        if (!mask[at] || !mask[at + (size_t)(dims[k] - 1) * st[k]]) { closed = false; break; }
      }
    if (!closed) {
      hc::set_error(std::string("hc_packing_set_walls: axis ") + "xyz"[k] + " is not periodic and has an open face: every node of both of its faces must be wall");
      return HC_ERR_ARG;
    }
  }

  // the field is needed as far as the largest wall cut-off at the first diameter reaches, margin and half a node included
  Ctl c;
  int rc = pk_read_ctl(P, &c);
  if (rc != HC_OK) return rc;
  std::vector<double> sizes(3 * (size_t)v.ns), pos(3 * (size_t)v.N);
  HC_HIP(hipMemcpy(sizes.data(), P->size.p, sizes.size() * sizeof(double), hipMemcpyDeviceToHost));
  HC_HIP(hipMemcpy(pos.data(), P->part.p, pos.size() * sizeof(double), hipMemcpyDeviceToHost));
  double amax = 0;
  for (double a : sizes) if (a > amax) amax = a;
  const double reach = (0.55 * c.Douter * amax + wall_margin) / spacing + 0.5;
  HC_REQUIRE(reach < 4000, "hc_packing_set_walls: the spacing is too fine for the particles (the distance field would reach past 4000 nodes)");
  const int R = (int)std::ceil(reach) + 1;
  for (int i = 0; i < v.N; i++) {
    size_t at = 0;
    bool out = false;
    for (int k = 0; k < 3; k++) {
      const double u = pos[(size_t)k * v.N + i] / spacing;
      if (!periodic[k] && !(u >= 0 && u <= dims[k] - 1)) { out = true; break; }
      int node = (int)std::floor(u + 0.5);
      node = periodic[k] ? ((node % dims[k]) + dims[k]) % dims[k] : (node > dims[k] - 1 ? dims[k] - 1 : node);
      at = at * dims[k] + node;
    }
    HC_REQUIRE(!out && !mask[at], "hc_packing_set_walls: a particle starts on a wall node or outside the mask");
  }

  hc::DevBuf<unsigned char> dmask;
  hc::DevBuf<int> g0, g1;
  if ((rc = dmask.reserve(n)) != HC_OK || (rc = g0.reserve(n)) != HC_OK || (rc = g1.reserve(n)) != HC_OK || (rc = P->snode.reserve(n)) != HC_OK ||
      (rc = P->wrec.reserve(7 * (size_t)v.N)) != HC_OK)
    return rc;
  HC_HIP(hipMemcpyAsync(dmask.p, mask, n, hipMemcpyHostToDevice, hc::stream()));
  const dim3 nb((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(pk_edt_init, nb, dim3(256), 0, hc::stream(), n, (const unsigned char *)dmask.p, g0.p);
  hipLaunchKernelGGL(pk_edt_pass, nb, dim3(256), 0, hc::stream(), n, (const int *)g0.p, g1.p, dims[0], dims[1], dims[2], 2, periodic[2] ? 1 : 0, R);
  hipLaunchKernelGGL(pk_edt_pass, nb, dim3(256), 0, hc::stream(), n, (const int *)g1.p, g0.p, dims[0], dims[1], dims[2], 1, periodic[1] ? 1 : 0, R);
  hipLaunchKernelGGL(pk_edt_pass, nb, dim3(256), 0, hc::stream(), n, (const int *)g0.p, g1.p, dims[0], dims[1], dims[2], 0, periodic[0] ? 1 : 0, R);
  hipLaunchKernelGGL(pk_edt_finish, nb, dim3(256), 0, hc::stream(), n, (const int *)g1.p, R, P->snode.p);
  HC_HIP(hipGetLastError());
  HC_HIP(hipStreamSynchronize(hc::stream()));   // dmask, g0 and g1 go out of scope

  v.walls = 1; v.wsp = spacing; v.wmargin = wall_margin; v.snode = P->snode; v.wrec = P->wrec;
  for (int k = 0; k < 3; k++) { v.wrap[k] = periodic[k] ? 1 : 0; v.wd[k] = dims[k]; }
  P->wall_R = R;
  // the calc_forces before the first iteration once more, now with the wall slot and the axes that no longer wrap; the
  // counters of the periodic evaluation that hc_packing_create ran are dropped
  HC_HIP(hipMemsetAsync(&P->ctl.p->maxeval, 0, 2 * sizeof(int), hc::stream()));   // maxeval, maxcount
  for (int attempt = 0;; attempt++) {
    pk_queue_forces(P, 1);
    HC_HIP(hipGetLastError());
    if ((rc = pk_read_ctl(P, &c)) != HC_OK) return rc;
    if (c.error) { hc::set_error("hc_packing_set_walls: a pair's root search did not end within 256 evaluations"); return HC_ERR_STATE; }
    if (!c.grow) break;
    if (attempt >= 4) { hc::set_error("hc_packing_set_walls: the pair lists did not settle"); return HC_ERR_STATE; }
    if ((rc = pk_grow(P, c)) != HC_OK) return rc;
  }
  return HC_OK;
}

int hc_packing_wall_field(hc_packing *P, double *s_node) {
  HC_REQUIRE(P && s_node, "hc_packing_wall_field: null pointer");
  HC_REQUIRE(P->v.walls, "hc_packing_wall_field: no walls are set");
  const size_t n = (size_t)P->v.wd[0] * P->v.wd[1] * P->v.wd[2];
  HC_HIP(hipMemcpyAsync(s_node, P->snode.p, n * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  return HC_OK;
}

int hc_packing_walls(int n, const double *size, const double *quat, const double *s, const double *normal, const double *douter2, int rotate,
                     double *force, double *torque, double *candidate, int *evals, int *kind) {
  HC_REQUIRE(n >= 0, "hc_packing_walls: n < 0");
  if (n == 0) return HC_OK;
  HC_REQUIRE(size && quat && s && normal && douter2 && force && torque && candidate && evals && kind, "hc_packing_walls: null pointer");
  std::vector<double> in(12 * (size_t)n), outv(7 * (size_t)n);
  std::vector<int> iout(3 * (size_t)n);
  for (int t = 0; t < n; t++) {
    double *x = &in[12 * (size_t)t];
    for (int k = 0; k < 3; k++) { x[k] = size[3 * t + k]; x[8 + k] = normal[3 * t + k]; }
    for (int k = 0; k < 4; k++) x[3 + k] = quat[4 * t + k];
    x[7] = s[t]; x[11] = douter2[t];
  }
  HC_REQUIRE(all_finite(in.data(), in.size()), "hc_packing_walls: non-finite input");
  hc::DevBuf<double> din, dout; hc::DevBuf<int> diout;
  int rc;
  if ((rc = din.reserve(in.size())) != HC_OK || (rc = dout.reserve(outv.size())) != HC_OK || (rc = diout.reserve(iout.size())) != HC_OK) return rc;
  HC_HIP(hipMemcpyAsync(din.p, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice, hc::stream()));
  hipLaunchKernelGGL(pk_wall_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hc::stream(), n, (const double *)din.p, rotate, dout.p, diout.p);
  HC_HIP(hipGetLastError());
  HC_HIP(hipMemcpyAsync(outv.data(), dout.p, outv.size() * sizeof(double), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipMemcpyAsync(iout.data(), diout.p, iout.size() * sizeof(int), hipMemcpyDeviceToHost, hc::stream()));
  HC_HIP(hipStreamSynchronize(hc::stream()));
  for (int t = 0; t < n; t++) {
    const double *y = &outv[7 * (size_t)t];
    for (int k = 0; k < 3; k++) { force[3 * t + k] = y[k]; torque[3 * t + k] = y[3 + k]; }
    candidate[t] = y[6];
    evals[t] = iout[3 * t + 1];
    kind[t] = iout[3 * t + 2] ? -1 : iout[3 * t];
  }
  return HC_OK;
}

int hc_packing_destroy(hc_packing *P) {
  if (!P) return HC_OK;
  (void)hipStreamSynchronize(hc::stream());
  delete P;
  return HC_OK;
}

}  // extern "C"
