// CPU restatement of the ellipsoid force-bias packing step (DESIGN §6 "packing"), for tests/packing_ref.py.
// Independent of hemocell_amd/csrc/packing.hip: no shared header.  Compiled by the tests with g++ -O2 -ffp-contract=off.
// It follows tools/packCells of the reference operation for operation (ellipsoid.h:303-405, packing.h:108-144, :345-428,
// :697-764, geometry.h) with the deviations the design lists: minimum image on both pair paths, sums in ascending partner
// index, the iprec table, a caller-given initial state, the root search capped at 256 evaluations, a step rotation that
// always has unit norm, and cell ranges taken by the floor modulo outside the box.
#include <cmath>
#include <cstring>
#include <vector>

namespace {

struct Vec { double v[3]; };
struct Mat { double m[3][3]; };

const int ROOT_CAP = 256;

double dot(const Vec &a, const Vec &b) { return a.v[0] * b.v[0] + a.v[1] * b.v[1] + a.v[2] * b.v[2]; }
Vec cross(const Vec &a, const Vec &b) {
  return Vec{{a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]}};
}
Vec scaled(const Vec &a, double d) { return Vec{{a.v[0] * d, a.v[1] * d, a.v[2] * d}}; }
// geometry.h:157-161
Vec unit(const Vec &a) {
  const double sp = dot(a, a);
  if (std::fabs(sp - 1) < 1e-10) return a;
  return scaled(a, 1 / std::sqrt(sp));
}
Mat zero() { Mat r; std::memset(&r, 0, sizeof r); return r; }
Mat mul(const Mat &a, const Mat &b) {   // geometry.h:186-198
  Mat r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return r;
}
Mat mscaled(const Mat &a, double d) { Mat r; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] * d; return r; }
Mat madd(const Mat &a, const Mat &b) { Mat r; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] + b.m[i][j]; return r; }
Mat msub(const Mat &a, const Mat &b) { Mat r; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] - b.m[i][j]; return r; }
Mat transposed(const Mat &a) { Mat r; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r.m[i][j] = a.m[j][i]; return r; }
Vec mvec(const Mat &a, const Vec &x) {
  Vec r;
  for (int i = 0; i < 3; i++) r.v[i] = a.m[i][0] * x.v[0] + a.m[i][1] * x.v[1] + a.m[i][2] * x.v[2];
  return r;
}
Mat adjugate(const Mat &a) {   // geometry.h:321-333
  const double(*m)[3] = a.m;
  Mat r;
  r.m[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
  r.m[0][1] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
  r.m[0][2] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  r.m[1][0] = m[0][2] * m[2][1] - m[2][2] * m[0][1];
  r.m[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
  r.m[1][2] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
  r.m[2][0] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
  r.m[2][1] = m[1][0] * m[0][2] - m[0][0] * m[1][2];
  r.m[2][2] = m[1][1] * m[0][0] - m[1][0] * m[0][1];
  return r;
}
double determinant(const Mat &a) {   // geometry.h:334-337
  const double(*m)[3] = a.m;
  return m[0][0] * m[1][1] * m[2][2] + m[1][0] * m[2][1] * m[0][2] + m[2][0] * m[0][1] * m[1][2] - m[0][2] * m[1][1] * m[2][0] -
         m[0][0] * m[1][2] * m[2][1] - m[0][1] * m[1][0] * m[2][2];
}
Mat inverse(const Mat &a) { return mscaled(adjugate(a), 1. / determinant(a)); }
double quad(const Mat &c, const Vec &x) {   // geometry.h:351-360
  const double(*m)[3] = c.m;
  const double *v = x.v;
  double w = m[0][0] * v[0] * v[0] + m[1][1] * v[1] * v[1] + m[2][2] * v[2] * v[2];
  w += m[0][1] * v[0] * v[1];
  w += m[0][2] * v[0] * v[2];
  w += m[1][0] * v[1] * v[0];
  w += m[1][2] * v[1] * v[2];
  w += m[2][0] * v[2] * v[0];
  w += m[2][1] * v[2] * v[1];
  return w;
}

struct Quat { double s; Vec p; };
// Quaternion(s, p) and norm(), geometry.h:386, 406-414
Quat make_quat(double s, const Vec &p) {
  Quat q{s, p};
  double sp = q.s * q.s + dot(q.p, q.p);
  if (std::fabs(sp - 1) > 1e-10) {
    sp = 1 / std::sqrt(sp);
    q.s *= sp;
    q.p = scaled(q.p, sp);
  }
  return q;
}
// a step's rotation: always to unit norm (the design's deviation 10; the reference's constructor skips it within 1e-10)
Quat unit_quat(double s, const Vec &p) {
  const double sp = 1 / std::sqrt(s * s + dot(p, p));
  return Quat{s * sp, scaled(p, sp)};
}
// geometry.h:400-405
Quat qmul(const Quat &t, const Quat &q) {
  Quat r;
  r.s = t.s * q.s - dot(t.p, q.p);
  const Vec c = cross(t.p, q.p);
  for (int k = 0; k < 3; k++) r.p.v[k] = (t.s * q.p.v[k] + q.s * t.p.v[k]) - c.v[k];
  return r;
}
// geometry.h:424-428
Mat rotation(const Quat &q) {
  Mat vv, sk = zero(), id = zero();
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) vv.m[i][j] = q.p.v[i] * q.p.v[j];
  sk.m[0][1] = -q.p.v[2]; sk.m[0][2] = q.p.v[1];
  sk.m[1][0] = q.p.v[2];  sk.m[1][2] = -q.p.v[0];
  sk.m[2][0] = -q.p.v[1]; sk.m[2][1] = q.p.v[0];
  id.m[0][0] = id.m[1][1] = id.m[2][2] = 1;
  return mscaled(madd(msub(vv, mscaled(sk, q.s)), mscaled(id, q.s * q.s - 0.5)), 2);
}
// ellipsoid.h:72-98: transp(Q) * diag * Q
Mat shape(const Quat &q, double d0, double d1, double d2) {
  Mat o = zero();
  o.m[0][0] = d0; o.m[1][1] = d1; o.m[2][2] = d2;
  const Mat Q = rotation(q);
  return mul(mul(transposed(Q), o), Q);
}
bool is_sphere(const double r[3]) { return std::fabs(r[0] - r[2]) < 1e-5 && std::fabs(r[0] - r[1]) < 1e-5; }   // ellipsoid.h:46

struct Contact {
  Mat XA_m1, XB_m1;
  Vec r;
  double p[5], q[4], h[7];
  double f(double l) const {
    return (p[0] + l * (p[1] + l * (p[2] + l * (p[3] + l * p[4])))) / (q[0] + l * (q[1] + l * (q[2] + l * q[3])));
  }
  double fd(double l) const { return h[0] + l * (h[1] + l * (h[2] + l * (h[3] + l * (h[4] + l * (h[5] + l * h[6]))))); }
};

// BinaryEllipsoidSystem, ellipsoid.h:316-364
Contact contact(const double ra[3], const Quat &qa, const double rb[3], const Quat &qb, const Vec &rij) {
  Contact c;
  c.XA_m1 = shape(qa, ra[0] * ra[0], ra[1] * ra[1], ra[2] * ra[2]);
  c.XB_m1 = shape(qb, rb[0] * rb[0], rb[1] * rb[1], rb[2] * rb[2]);
  const Mat XB_12 = shape(qb, 1 / rb[0], 1 / rb[1], 1 / rb[2]);
  c.r = rij;
  const Mat A = mul(mul(XB_12, c.XA_m1), XB_12);
  const Vec a = mvec(XB_12, rij);
  const double detA = determinant(A);
  const Mat Z = adjugate(A);
  Mat C1 = mscaled(Z, -2), C2 = Z;
  C1.m[0][0] += A.m[1][1] + A.m[2][2];
  C1.m[1][1] += A.m[0][0] + A.m[2][2];
  C1.m[2][2] += A.m[1][1] + A.m[0][0];
  C2.m[0][0] -= A.m[1][1] + A.m[2][2] - 1;
  C2.m[1][1] -= A.m[0][0] + A.m[2][2] - 1;
  C2.m[2][2] -= A.m[1][1] + A.m[0][0] - 1;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      if (i != j) { C1.m[i][j] -= A.m[j][i]; C2.m[i][j] += A.m[j][i]; }
  const double w0 = quad(Z, a), w1 = quad(C1, a), w2 = quad(C2, a);
  const double sa = A.m[0][0] + A.m[1][1] + A.m[2][2];
  const double sz = Z.m[0][0] + Z.m[1][1] + Z.m[2][2];
  double *p = c.p, *q = c.q, *h = c.h;
  if (std::fabs(detA) > 1e-5) {
    p[0] = 0; p[1] = w0; p[2] = w1 - w0; p[3] = w2 - w1; p[4] = -w2;
    q[0] = detA; q[1] = -3 * detA + sz; q[2] = 3 * detA + sa - 2 * sz; q[3] = 1 - detA - sa + sz;
    h[0] = q[0] * p[1];
    h[1] = 2 * q[0] * p[2];
    h[2] = 3 * q[0] * p[3] + q[1] * p[2] - q[2] * p[1];
    h[3] = 4 * q[0] * p[4] + 2 * q[1] * p[3] - 2 * q[3] * p[1];
    h[4] = 3 * q[1] * p[4] + q[2] * p[3] - q[3] * p[2];
    h[5] = 2 * q[2] * p[4];
    h[6] = q[3] * p[4];
  } else {
    p[0] = w0; p[1] = w1 - w0; p[2] = w2 - w1; p[3] = -w2; p[4] = 0;
    q[0] = sz; q[1] = sa - 2 * sz; q[2] = 1 - sa + sz; q[3] = 0;
    h[0] = q[0] * p[1];
    h[1] = 2 * q[0] * p[2];
    h[2] = 3 * q[0] * p[3] + q[1] * p[2] - q[2] * p[1];
    h[3] = 2 * q[1] * p[3];
    h[4] = q[2] * p[3];
    h[5] = 0; h[6] = 0;
  }
  return c;
}

// zeroin on [0, 1], packing.h:697-764, with the evaluation cap; *evals counts f_AB_d calls, capped = 1 when the cap ended it
double root(const Contact &e, int *evals, int *capped) {
  const double EPSILON = 1e-15, tol = 0.0;
  double a = 0., b = 1., c = a;
  double fa = e.fd(a), fb = e.fd(b), fc = fa;
  int n = 2;
  *capped = 0;
  for (;;) {
    const double prev_step = b - a;
    double p, q, new_step;
    if (std::fabs(fc) < std::fabs(fb)) { a = b; b = c; c = a; fa = fb; fb = fc; fc = fa; }
    const double tol_act = 2 * EPSILON * std::fabs(b) + tol / 2;
    new_step = (c - b) / 2;
    if (std::fabs(new_step) <= tol_act || fb == 0.) break;
    if (n >= ROOT_CAP) { *capped = 1; break; }
    if (std::fabs(prev_step) >= tol_act && std::fabs(fa) > std::fabs(fb)) {
      double t1, t2;
      const double cb = c - b;
      if (a == c) {
        t1 = fb / fa;
        p = cb * t1;
        q = 1.0 - t1;
      } else {
        q = fa / fc;
        t1 = fb / fc;
        t2 = fb / fa;
        p = t2 * (cb * q * (q - t1) - (b - a) * (t1 - 1.0));
        q = (q - 1.0) * (t1 - 1.0) * (t2 - 1.0);
      }
      if (p > 0.) q = -q; else p = -p;
      if (p < (0.75 * cb * q - std::fabs(tol_act * q) / 2) && p < std::fabs(prev_step * q / 2)) new_step = p / q;
    }
    if (std::fabs(new_step) < tol_act) new_step = new_step > 0. ? tol_act : -tol_act;
    a = b; fa = fb;
    b += new_step;
    fb = e.fd(b);
    n++;
    if ((fb > 0 && fc > 0) || (fb < 0 && fc < 0)) { c = a; fc = fa; }
  }
  *evals = n;
  return b;
}

struct PairOut {
  int kind;   // 0: lambda too small or capped (nothing), 1: no overlap, 2: overlap
  int evals, capped;
  double lambda, fscl;
  Vec n, f, tA, tB;   // f: what B gains and A loses; tA, tB: the unsigned torque terms
};

// Packing::calc_forces(e, ei, ej), packing.h:108-144
PairOut pair(const double ra[3], const Quat &qa, const double rb[3], const Quat &qb, const Vec &rij, double Douter2, int rotate) {
  PairOut o;
  std::memset(&o, 0, sizeof o);
  const Contact e = contact(ra, qa, rb, qb, rij);
  const double lambda = root(e, &o.evals, &o.capped);
  o.lambda = lambda;
  if (o.capped || std::fabs(lambda) < 1e-10) return o;
  o.fscl = 4 * e.f(lambda);
  const double f_AB = o.fscl / Douter2;
  const Mat Y = madd(mscaled(e.XB_m1, lambda), mscaled(e.XA_m1, 1 - lambda));
  o.n = mvec(inverse(Y), e.r);
  o.kind = 1;
  if (f_AB >= 1) return o;
  o.kind = 2;
  o.f = scaled(unit(o.n), 1 - f_AB);
  if (!rotate) return o;
  if (!is_sphere(ra)) o.tA = scaled(unit(cross(mvec(mscaled(e.XA_m1, 1 - lambda), o.n), o.n)), 1 - f_AB);
  if (!is_sphere(rb)) o.tB = scaled(unit(cross(mvec(mscaled(e.XB_m1, -lambda), o.n), o.n)), 1 - f_AB);
  return o;
}

const double POW10_NEG[16] = {1e-0, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12, 1e-13, 1e-14, 1e-15};

struct Sim {
  int N, ns, grid[3], ncell_min, rotate;
  std::vector<double> size;   // [ns][3]
  std::vector<int> spec;      // [N]
  std::vector<Vec> pos, f, fu;
  std::vector<Quat> q;
  double box[3], half[3];
  double Diam_dens, Douter0, Douter, Douter2, Relax, Dinner, Force_step, Pactual, DensityNominal, Epsilon, Epsilon_rot, Rc_max;
  int Nsf, doExit, finished, steps, error, maxeval;
  long npairs;

  Vec sep(int A, int B) const {   // pos_B - pos_A, then pbc_diff (geometry.h:113-121)
    Vec r;
    for (int k = 0; k < 3; k++) {
      double d = pos[B].v[k] - pos[A].v[k];
      if (d < -half[k]) d += box[k]; else if (d > half[k]) d -= box[k];
      r.v[k] = d;
    }
    return r;
  }
  // packing.h:387-395, :438-463: is B < A a partner of A?  B has a cell only where (int)x lies in 0..grid-1, and A's range is
  // taken by the floor modulo, so that it stays a range of cells once x + grid - Rcut is negative (the design's deviation 11)
  bool active(int A, int B) const {
    const double Rcut = 0.55 * Douter * (size[3 * spec[A]] + Rc_max);
    if (!((int)(2.0 * Rcut) < ncell_min - 1)) return true;
    for (int k = 0; k < 3; k++) {
      const int low = (int)(pos[A].v[k] + grid[k] - Rcut), lim = (int)(pos[A].v[k] + grid[k] + Rcut);
      const int c = (int)pos[B].v[k];
      if (c < 0 || c >= grid[k]) return false;   // the reference would index past its cell array
      bool in = false;
      for (int leap = low; leap <= lim; leap++) if ((leap % grid[k] + grid[k]) % grid[k] == c) in = true;
      if (!in) return false;
    }
    return true;
  }
  void forces() {   // packing.h:370-397
    double dmin = Douter * Douter;
    for (int i = 0; i < N; i++) f[i] = fu[i] = Vec{{0, 0, 0}};
    npairs = 0;
    for (int A = 0; A < N; A++)
      for (int B = 0; B < A; B++) {
        if (!active(A, B)) continue;
        npairs++;
        const PairOut o = pair(&size[3 * spec[A]], q[A], &size[3 * spec[B]], q[B], sep(A, B), Douter2, rotate);
        if (o.evals > maxeval) maxeval = o.evals;
        if (o.capped) error = 1;
        if (o.kind != 2) continue;
        if (o.fscl < dmin) dmin = o.fscl;
        for (int k = 0; k < 3; k++) {
          f[A].v[k] -= o.f.v[k]; f[B].v[k] += o.f.v[k];
          fu[A].v[k] -= o.tA.v[k]; fu[B].v[k] += o.tB.v[k];
        }
      }
    Dinner = std::sqrt(dmin);
  }
  void motion() {   // packing.h:399-428
    const double eps = Epsilon * Douter0;
    Force_step = 0;
    for (int i = 0; i < N; i++) {
      Force_step += std::sqrt(dot(f[i], f[i]));
      for (int k = 0; k < 3; k++) {
        double x = pos[i].v[k] + f[i].v[k] * eps;
        if (x < 0) x += box[k]; else if (x > box[k]) x -= box[k];
        pos[i].v[k] = x;
      }
      if (!rotate || is_sphere(&size[3 * spec[i]])) continue;
      const double len = Epsilon_rot * std::sqrt(dot(fu[i], fu[i]));
      const double cp = 1 / std::sqrt(1 + len * len);
      const double sp = len * cp;
      const double cp2 = std::sqrt(0.5 * (1 + cp));
      const double sp2 = 0.5 * sp / cp2;
      q[i] = qmul(q[i], unit_quat(cp2, scaled(fu[i], sp2)));
    }
    Force_step /= N;
  }
  void iterate() {   // packing.h:345-368
    Douter -= Relax;
    Douter2 = Douter * Douter;
    motion();
    forces();
    DensityNominal = Douter * Douter * Douter / Diam_dens;
    Pactual = Dinner * Dinner * Dinner / Diam_dens;
    steps++;
    finished = Force_step < 1e-15;
    if (finished || doExit) return;
    const double d = DensityNominal - Pactual;
    if (d > 0 && d <= POW10_NEG[Nsf]) {
      Relax *= 0.5;
      if (++Nsf >= 16) doExit = 1;
    }
  }
};

}  // namespace

extern "C" {

// out: lambda, fscl, n[3], fA[3], tA[3], fB[3], tB[3] (17 doubles); flags: kind, evals, capped.  qa, qb = (s, p) before normalising.
void pkref_pair(const double *ra, const double *qa, const double *rb, const double *qb, const double *rij, double Douter2, int rotate,
                double *out, int *flags) {
  const Quat A = make_quat(qa[0], Vec{{qa[1], qa[2], qa[3]}}), B = make_quat(qb[0], Vec{{qb[1], qb[2], qb[3]}});
  const PairOut o = pair(ra, A, rb, B, Vec{{rij[0], rij[1], rij[2]}}, Douter2, rotate);
  out[0] = o.lambda; out[1] = o.fscl;
  const Vec zero3{{0, 0, 0}};
  for (int k = 0; k < 3; k++) {
    out[2 + k] = o.n.v[k];
    out[5 + k] = zero3.v[k] - o.f.v[k];
    out[8 + k] = zero3.v[k] - o.tA.v[k];
    out[11 + k] = zero3.v[k] + o.f.v[k];
    out[14 + k] = zero3.v[k] + o.tB.v[k];
  }
  flags[0] = o.kind; flags[1] = o.evals; flags[2] = o.capped;
}

void *pkref_create(const int *grid, int ns, const double *sizes, const int *counts, const double *pos, const double *quat,
                   double nominal, int rotate, int ntau, double epsilon) {
  Sim *S = new Sim;
  S->ns = ns; S->rotate = rotate;
  S->size.assign(sizes, sizes + 3 * ns);
  S->N = 0;
  for (int s = 0; s < ns; s++) for (int c = 0; c < counts[s]; c++) { S->spec.push_back(s); S->N++; }
  const int N = S->N;
  for (int k = 0; k < 3; k++) { S->grid[k] = grid[k]; S->box[k] = grid[k]; S->half[k] = 0.5 * S->box[k]; }
  S->ncell_min = grid[0] < grid[1] ? grid[0] : grid[1];
  if (grid[2] < S->ncell_min) S->ncell_min = grid[2];
  S->pos.resize(N); S->f.resize(N); S->fu.resize(N); S->q.resize(N);
  for (int i = 0; i < N; i++) {
    S->pos[i] = Vec{{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}};
    S->q[i] = quat ? Quat{quat[4 * i], Vec{{quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3]}}} : Quat{1, Vec{{0, 0, 0}}};
  }
  // Packing::init, packing.h:265-290
  const int No_cells = grid[0] * grid[1] * grid[2];
  S->Diam_dens = No_cells / (3.141592653589793 / 6.);
  double corr = 0;
  S->Rc_max = 0;
  for (int s = 0; s < ns; s++) { corr += counts[s]; if (sizes[3 * s] > S->Rc_max) S->Rc_max = sizes[3 * s]; }
  S->Diam_dens /= corr;
  S->DensityNominal = nominal;
  S->Douter0 = std::pow(S->Diam_dens * nominal, 1. / 3.);
  S->Douter = S->Douter0;
  S->Relax = 0.5 * S->Douter / ntau;
  S->Douter2 = S->Douter * S->Douter;
  S->Epsilon = epsilon;
  const double alpha = sizes[0];
  S->Epsilon_rot = 50. / (alpha * alpha * alpha);
  S->Nsf = 1; S->doExit = 0; S->finished = 0; S->steps = 0; S->error = 0; S->maxeval = 0; S->Force_step = 0;
  S->forces();   // execute(), packing.h:179-182
  S->Pactual = S->Dinner * S->Dinner * S->Dinner / S->Diam_dens;
  return S;
}

void pkref_run(void *h, int max_steps) {
  Sim *S = (Sim *)h;
  for (int k = 0; k < max_steps && !S->finished && !S->error; k++) S->iterate();
}

// status: steps, finished, Douter, Dinner, Pactual, DensityNominal, Force_step, Relax, Nsf, error, maxeval, pairs of the last step
void pkref_status(void *h, double *st) {
  const Sim *S = (const Sim *)h;
  st[0] = S->steps; st[1] = S->finished; st[2] = S->Douter; st[3] = S->Dinner; st[4] = S->Pactual; st[5] = S->DensityNominal;
  st[6] = S->Force_step; st[7] = S->Relax; st[8] = S->Nsf; st[9] = S->error; st[10] = S->maxeval; st[11] = (double)S->npairs;
}

void pkref_state(void *h, double *pos, double *quat, double *force, double *torque) {
  const Sim *S = (const Sim *)h;
  for (int i = 0; i < S->N; i++) {
    for (int k = 0; k < 3; k++) { pos[3 * i + k] = S->pos[i].v[k]; force[3 * i + k] = S->f[i].v[k]; torque[3 * i + k] = S->fu[i].v[k]; }
    quat[4 * i] = S->q[i].s;
    for (int k = 0; k < 3; k++) quat[4 * i + 1 + k] = S->q[i].p.v[k];
  }
}

void pkref_destroy(void *h) { delete (Sim *)h; }

// brute force over all pairs with the minimum image: the smallest f_AB = 4 f(lambda) / Douter2 and the number of pairs below 1.
// Pairs whose root search gives nothing (lambda too small, cap) count in *skipped.
double pkref_min_contact(const int *grid, int ns, const double *sizes, const int *counts, const double *pos, const double *quat,
                         double Douter, int *overlapping, int *skipped) {
  std::vector<int> spec;
  for (int s = 0; s < ns; s++) for (int c = 0; c < counts[s]; c++) spec.push_back(s);
  const int N = (int)spec.size();
  double best = HUGE_VAL;
  *overlapping = 0; *skipped = 0;
  for (int A = 0; A < N; A++)
    for (int B = 0; B < A; B++) {
      Vec r;
      for (int k = 0; k < 3; k++) {
        double d = pos[3 * B + k] - pos[3 * A + k];
        const double box = grid[k], half = 0.5 * box;
        if (d < -half) d += box; else if (d > half) d -= box;
        r.v[k] = d;
      }
      const Quat qa{quat[4 * A], Vec{{quat[4 * A + 1], quat[4 * A + 2], quat[4 * A + 3]}}};
      const Quat qb{quat[4 * B], Vec{{quat[4 * B + 1], quat[4 * B + 2], quat[4 * B + 3]}}};
      const PairOut o = pair(&sizes[3 * spec[A]], qa, &sizes[3 * spec[B]], qb, r, Douter * Douter, 0);
      if (o.kind == 0) { (*skipped)++; continue; }
      const double fab = o.fscl / (Douter * Douter);
      if (fab < best) best = fab;
      if (fab < 1) (*overlapping)++;
    }
  return best;
}

}  // extern "C"
