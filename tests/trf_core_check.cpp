// Host check of the trf solver's scalar core (csrc/lsmr_dev.hpp, csrc/trf_host.hpp, which optim_trf.hip runs), on small
// dense problems, without HIP: tests/test_trf_core.py writes the problems, runs this program and compares its
// answers with oracle/trf.py.
//
//   trf_core_check IN OUT
// IN, whitespace-separated:
//   lsmr m n damp maxiter tol conlim  A (m n, row-major)  b (m)   -> OUT: lsmr istop itn x (n)   (atol = btol = tol)
//   trf kind ftol max_nfev nd data (nd) n x0 (n)             -> OUT: trf status nfev njev cost x (n)
// kind 0: r_i = x0 exp(x1 t_i) + x2 - y_i, data = t (nd / 2) then y;  kind 1: r = (10 (x1 - x0^2), 1 - x0).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lsmr_dev.hpp"
#include "trf_host.hpp"

using Vec = std::vector<double>;

static double dot(const Vec& a, const Vec& b) {
  double s = 0.0;
  for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
  return s;
}
struct Dense {  // row-major m x n
  int m = 0, n = 0;
  Vec a;
  Vec mul(const Vec& v, double vs) const {  // A (v vs)
    Vec o(m, 0.0);
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < n; ++c) o[r] += a[(size_t)r * n + c] * (v[c] * vs);
    return o;
  }
  Vec tmul(const Vec& u, double us) const {  // A^T (u us)
    Vec o(n, 0.0);
    for (int r = 0; r < m; ++r)
      for (int c = 0; c < n; ++c) o[c] += a[(size_t)r * n + c] * (u[r] * us);
    return o;
  }
};

// lsmr(A, b, damp) in the kernels' phase order: per iteration k the u phase (iteration k - 1's recurrences and
// x / h / hbar updates, then u = A v - alpha u), then the v phase (iteration k - 1's stop test, then
// v = A^T u - beta v); vectors raw, scaled by 1 / norm where they are read.  Returns istop (8: the x = 0 exit).
static int lsmr_dense(const Dense& A, const Vec& b, double damp, double maxiter, double tol, double conlim, Vec& x,
                      double& itn) {
  const int n = A.n;
  const double normb = std::sqrt(dot(b, b));
  Vec u = b, vraw = A.tmul(b, normb > 0 ? 1 / normb : 0.0), vn(n), h(n), hbar(n, 0.0);
  x.assign(n, 0.0);
  double S[mq::LSMR_NS], vv = dot(vraw, vraw), uu = 0.0, xx = 0.0;
  for (int k = 1;; ++k) {
    const double alpha = std::sqrt(vv), beta = k == 1 ? normb : std::sqrt(uu);
    double chb = 0.0, cx = 0.0, ch = 0.0;
    if (k == 1) {
      if (mq::lsmr_start(S, alpha, beta, damp)) {
        itn = 0;
        return 8;
      }
    } else {
      mq::lsmr_recurrence(S, alpha, beta, damp, chb, cx, ch);
    }
    const double ia = 1 / alpha;
    xx = 0.0;
    for (int i = 0; i < n; ++i) {
      vn[i] = vraw[i] * ia;
      if (k == 1) {
        h[i] = vn[i];
      } else {
        hbar[i] = hbar[i] * chb + h[i];
        x[i] = x[i] + cx * hbar[i];
        h[i] = h[i] * ch + vn[i];
        xx += x[i] * x[i];
      }
    }
    const Vec av = A.mul(vraw, ia);
    for (int r = 0; r < A.m; ++r) u[r] = (u[r] * (1 / beta)) * -alpha + av[r];
    uu = dot(u, u);
    const double betak = std::sqrt(uu);
    if (k > 1) {
      const int istop = mq::lsmr_istop(S, std::sqrt(xx), normb, maxiter, tol, tol, 1.0 / conlim);
      if (istop) {
        itn = S[mq::S_ITN];
        return istop;
      }
    }
    const Vec atu = A.tmul(u, 1 / betak);
    for (int i = 0; i < n; ++i) vraw[i] = vn[i] * -betak + atu[i];
    vv = dot(vraw, vraw);
  }
}

// the toy least-squares problems: residuals and the analytic Jacobian
struct Toy {
  int kind = 0;
  Vec data;
  void eval(const Vec& x, Vec& f, Dense& J) const {
    if (kind == 0) {
      const int m = (int)data.size() / 2;
      f.resize(m);
      J.m = m, J.n = 3, J.a.resize((size_t)m * 3);
      for (int i = 0; i < m; ++i) {
        const double e = std::exp(x[1] * data[i]);
        f[i] = x[0] * e + x[2] - data[m + i];
        J.a[3 * i] = e, J.a[3 * i + 1] = x[0] * data[i] * e, J.a[3 * i + 2] = 1.0;
      }
    } else {
      f = {10 * (x[1] - x[0] * x[0]), 1 - x[0]};
      J.m = 2, J.n = 2, J.a = {-20 * x[0], 10.0, -1.0, 0.0};
    }
  }
};

// trf_no_bounds (trf.py:401-540) as the drivers run it: mq::TrfAnimal between the dense stand-ins of their launches
static void trf_dense(const Toy& toy, Vec& x, double ftol, long long max_nfev, mq::TrfAnimal& a) {
  const int n = (int)x.size();
  Vec f, g, ft, gn, s1(n), s2(n), xt(n);
  Dense J, Jt;
  auto read_jac = [&]() {  // the drivers' read_jac: what the loop needs at an x it keeps
    a.cost = 0.5 * dot(f, f);
    a.rows = J.m;
    g = J.tmul(f, 1.0);
    a.gnorm2 = dot(g, g);
    a.ginf = 0.0;
    for (double v : g) a.ginf = std::max(a.ginf, std::fabs(v));
    a.xnorm = std::sqrt(dot(x, x));
    const Vec jg = J.mul(g, 1.0);
    a.areg = 0.5 * dot(jg, jg);
  };
  toy.eval(x, f, J);
  read_jac();
  a.start(max_nfev > 0 ? max_nfev : 100LL * n);
  while (a.begin_iteration()) {
    double damp, maxiter, itn;
    a.lsmr_setup(n, damp, maxiter);
    lsmr_dense(J, f, damp, maxiter, 1e-6, 1e8, gn, itn);  // least_squares' lsmr tolerances
    a.record_lsmr(itn);
    // S = orth([g, gn]) by Gram-Schmidt, g_S and B_S (trf.py:489-493)
    const double ng = std::sqrt(a.gnorm2), proj = ng > 0 ? dot(g, gn) / ng : 0.0;
    for (int i = 0; i < n; ++i) s1[i] = ng > 0 ? g[i] / ng : 0.0, s2[i] = gn[i] - proj * s1[i];
    const double nw = std::sqrt(dot(s2, s2));
    for (int i = 0; i < n; ++i) s2[i] = nw > 0 ? s2[i] / nw : 0.0;
    const Vec j1 = J.mul(s1, 1.0), j2 = J.mul(s2, 1.0);
    a.g_S[0] = dot(s1, g), a.g_S[1] = dot(s2, g);
    a.B_S[0] = dot(j1, j1), a.B_S[1] = dot(j1, j2), a.B_S[2] = dot(j2, j2);
    double p[2];
    while (a.propose_trial(p)) {
      double st = 0.0;
      for (int i = 0; i < n; ++i) {
        const double step = s1[i] * p[0] + s2[i] * p[1];
        xt[i] = x[i] + step;
        st += step * step;
      }
      toy.eval(xt, ft, Jt);
      a.judge_trial(std::sqrt(st), 0.5 * dot(ft, ft), ftol);
    }
    if (a.accept()) {
      x = xt, f = ft, J = Jt;
      read_jac();
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  auto num = [&]() {
    double v = 0.0;
    if (fscanf(in, "%lf", &v) != 1) std::exit(3);
    return v;
  };
  auto vec = [&](int n) {
    Vec v(n);
    for (double& e : v) e = num();
    return v;
  };
  auto put = [&](const Vec& v) {
    for (double e : v) fprintf(out, " %.17g", e);
    fprintf(out, "\n");
  };
  char word[16];
  while (fscanf(in, "%15s", word) == 1) {
    if (!strcmp(word, "lsmr")) {
      Dense A;
      A.m = (int)num(), A.n = (int)num();
      const double damp = num(), maxiter = num(), tol = num(), conlim = num();
      A.a = vec(A.m * A.n);
      const Vec b = vec(A.m);
      Vec x;
      double itn = 0.0;
      const int istop = lsmr_dense(A, b, damp, maxiter, tol, conlim, x, itn);
      fprintf(out, "lsmr %d %d", istop, (int)itn);
      put(x);
    } else if (!strcmp(word, "trf")) {
      Toy toy;
      toy.kind = (int)num();
      const double ftol = num();
      const long long max_nfev = (long long)num();
      toy.data = vec((int)num());
      Vec x = vec((int)num());
      mq::TrfAnimal a;
      trf_dense(toy, x, ftol, max_nfev, a);
      double st[8] = {};
      a.write_stats(st);
      fprintf(out, "trf %d %d %d %.17g", (int)st[3], (int)st[4], (int)st[5], st[1]);
      put(x);
    } else {
      return 4;
    }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 5;
}
