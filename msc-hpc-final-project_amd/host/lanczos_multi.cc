// lanczos_multi.cc -- lanczosDecompMulti (see lanczos_multi.h).
#include "lanczos_multi.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "SPMV.h"
#include "cu_lanczos.h"
#include "eigen.h"
#include "lzx.h"

namespace {
void lzx_or_throw(int rc, const char *what) {
  if (rc != LZX_OK) throw std::runtime_error(std::string(what) + ": " + lzx_last_error());
}
}  // namespace

lanczosDecompMulti::lanczosDecompMulti(adjMatrix &adj, unsigned krylov, const double *Xin, unsigned nb, bool on_gpu)
    : lanczosDecompMulti(adj, krylov, Xin, nb, on_gpu, graphOperator::adjacency, 1.0) {}

lanczosDecompMulti::lanczosDecompMulti(adjMatrix &adj, unsigned krylov, const double *Xin, unsigned nb, bool on_gpu, graphOperator o,
                                       double t)
    : A{adj}, krylov_dim{krylov}, b{nb}, cuda{on_gpu}, op{o}, time{t} {
  if (krylov == 0) throw std::invalid_argument("lanczosDecompMulti: krylov dimension must be positive");
  if (nb == 0) throw std::invalid_argument("lanczosDecompMulti: no starting vectors");
  const std::size_t n = A.get_n(), k = krylov;
  X.assign(Xin, Xin + n * nb);
  alpha.assign(nb * k, 0.0);
  beta.assign(nb * k, 0.0);
  xn.assign(nb, 0.0);
  kused.assign(nb, 0);
  ans.assign(n * nb, 0.0);
  answered.assign(nb, 0);
  if (!cuda) {
    Q.assign(nb * k * n, 0.0);
    for (unsigned c = 0; c < nb; ++c) decompose_column(c);
    return;
  }
  graph = A.device_graph();
  if (graph->ranks.size() != 1)
    throw std::runtime_error("lanczosDecompMulti: the batched path is one-GPU; this graph is spread over " +
                             std::to_string(graph->ranks.size()) + " GPU handles (LZX_DEVICES)");
  // every batch but the last is answered before the next one overwrites the resident batch basis
  for (unsigned first = 0; first < nb; first += batch) {
    run_batch(first);
    if (first + batch < nb) answer_batch(first);
  }
}

lanczosDecompMulti::~lanczosDecompMulti() {
  if (graph && graph->multi_owner == this) graph->multi_owner = nullptr;
}

// decompose() (lanczos.cc) for column c, with the breakdown stop: after beta_j (j < k - 1) the column stops when
// beta_j <= 2^-40 * max_{i<=j} (|alpha_i| + beta_{i-1}); later alpha / beta / basis vectors stay 0, k_used = j + 1.
void lanczosDecompMulti::decompose_column(unsigned c) {
  const unsigned n = A.get_n(), k = krylov_dim;
  double *a = alpha.data() + static_cast<std::size_t>(c) * k, *bt = beta.data() + static_cast<std::size_t>(c) * k;
  double *Qc = Q.data() + static_cast<std::size_t>(c) * k * n;
  const double *x = X.data() + static_cast<std::size_t>(c) * n;
  std::vector<double> v(n), cur(n), prev(n);
  const double xnorm = norm(x, n);
  xn[c] = xnorm;
  for (unsigned r = 0; r < n; ++r) cur[r] = x[r] / xnorm;
  double mx = 0.0;
  kused[c] = k;
  const bool lap = op == graphOperator::laplacian;
  double lstop = 0.0;   // under L: 2^-40 * 2 d_max (lanczos.cc: breakdown)
  if (lap) {
    unsigned dmax = 0;
    for (unsigned r = 0; r < n; ++r) dmax = std::max(dmax, A.row_offset[r + 1] - A.row_offset[r]);
    lstop = std::ldexp(2.0 * dmax, -40);
  }
  for (unsigned j = 0; j < k; ++j) {
    spMV(A, cur.data(), v.data());
    if (lap)
      for (unsigned r = 0; r < n; ++r) v[r] = std::fma(static_cast<double>(A.row_offset[r + 1] - A.row_offset[r]), cur[r], -v[r]);
    a[j] = inner_prod(v.data(), cur.data(), n);
    for (unsigned r = 0; r < n; ++r) v[r] -= a[j] * cur[r];
    if (j > 0)
      for (unsigned r = 0; r < n; ++r) v[r] -= bt[j - 1] * prev[r];
    std::copy(cur.begin(), cur.end(), Qc + static_cast<std::size_t>(j) * n);
    if (j + 1 < k) {
      const double nb = norm(v.data(), n);
      mx = std::max(mx, std::abs(a[j]) + (j > 0 ? bt[j - 1] : 0.0));
      if (lap ? nb <= lstop : nb <= 0x1p-40 * mx) {
        kused[c] = j + 1;
        return;
      }
      bt[j] = nb;
      for (unsigned r = 0; r < n; ++r) prev[r] = v[r] / bt[j];
      cur.swap(prev);
    }
  }
}

void lanczosDecompMulti::run_batch(unsigned first) {
  const std::size_t n = A.get_n(), k = krylov_dim;
  const unsigned cnt = std::min(batch, b - first);
  lzx_stats st{};
  lzx_or_throw(lzx_set_option(graph->ranks[0], "operator", op == graphOperator::laplacian ? LZX_OP_LAPLACIAN : LZX_OP_ADJACENCY),
               "lzx_set_option(operator)");
  lzx_or_throw(lzx_lanczos_multi_f64(graph->ranks[0], cnt, X.data() + first * n, krylov_dim, alpha.data() + first * k,
                                     beta.data() + first * k, kused.data() + first, xn.data() + first, nullptr, &st),
               "lzx_lanczos_multi_f64");
  graph->multi_owner = this;
  graph->multi_first = first;
  loop_ms_ += st.loop_ms;
}

void lanczosDecompMulti::answer_batch(unsigned first) {
  const std::size_t n = A.get_n(), k = krylov_dim;
  const unsigned cnt = std::min(batch, b - first);
  std::vector<double> T(cnt * k, 0.0), d, e, z;
  for (unsigned i = 0; i < cnt; ++i) {
    const unsigned c = first + i, ku = kused[c];
    // t = V (e^{s lambda} .* ||x|| V[0,:]) of the leading k_used x k_used block (multiplyOut.cc: small_part); s = time under A
    // (1: e^lambda bit for bit), -time under L
    d.assign(alpha.begin() + c * k, alpha.begin() + c * k + ku);
    e.assign(ku, 0.0);
    for (unsigned j = 0; j + 1 < ku; ++j) e[j] = beta[c * k + j];
    z.assign(static_cast<std::size_t>(ku) * ku, 0.0);
    if (symtridiag_ql(static_cast<int>(ku), d.data(), e.data(), z.data()) != 0)
      throw std::runtime_error("lanczosDecompMulti: QL iteration did not converge");
    const double es = op == graphOperator::laplacian ? -time : time;
    for (unsigned j = 0; j < ku; ++j) d[j] = std::exp(d[j] * es) * (xn[c] * z[j]);
    double *t = T.data() + i * k;
    for (unsigned r = 0; r < ku; ++r) {
      double s = 0;
      for (unsigned j = 0; j < ku; ++j) s += z[static_cast<std::size_t>(r) * ku + j] * d[j];
      t[r] = s;
    }
    if (!cuda) {
      double *out = ans.data() + c * n;
      std::fill(out, out + n, 0.0);
      for (unsigned j = 0; j < ku; ++j) {
        const double *q = Q.data() + (c * k + j) * n;
        for (std::size_t r = 0; r < n; ++r) out[r] += t[j] * q[r];
      }
    }
  }
  if (cuda) {
    // another batched decomposition on this graph may have overwritten the resident basis since: this batch again (same bits)
    if (graph->multi_owner != this || graph->multi_first != first) run_batch(first);
    lzx_or_throw(lzx_multout_multi_f64(graph->ranks[0], cnt, T.data(), krylov_dim, ans.data() + first * n), "lzx_multout_multi_f64");
  }
  for (unsigned i = 0; i < cnt; ++i) answered[first + i] = 1;
}

void multOutMulti(lanczosDecompMulti &L, adjMatrix &) {
  for (unsigned first = 0; first < L.b; first += lanczosDecompMulti::batch)
    if (!L.answered[first]) L.answer_batch(first);
}
