// lanczos_multi.h -- `lanczosDecompMulti`: e^A x for b starting vectors at once, as b independent Lanczos decompositions
// (one three-term recurrence per column of X, no coupling between them -- not block Lanczos), on the CPU (cuda == false) or
// on one MI355X through the lzx C ABI's batched path (cuda == true: lzx_lanczos_multi_f64, which shares ONE SpMM per iteration
// among up to 16 columns; more columns run as several batches).
//
// Each column stops on its own when its Krylov space is exhausted (include/lzx.h: beta_j <= 2^-40 * max_{i<=j}(|alpha_i| +
// beta_{i-1})): a seed vector e_v of a small component then uses k_used <= its size instead of dividing by a rounding-level
// beta.  The CPU path is decompose() of lanczos.cc per column with that stop (bit-identical alpha / beta where it does not
// fire); decompose() itself is unchanged.
//
//   lanczosDecompMulti L(A, k, X, b, cuda);   // X: b contiguous vectors of n
//   multOutMulti(L, A);                         // L.answer(): b contiguous vectors e^A x_c
//
// multOutMulti solves each column's k_used x k_used tridiagonal matrix with the QL solver of eigen.cc and forms Q_c t_c: on the
// host (CPU path) or on the device-resident batch basis.  On the device only the last batch's basis stays resident, so the
// constructor forms the answers of the earlier batches before the next one overwrites it.  One GPU only: a device graph
// spread over several handles (LZX_DEVICES) makes the constructor throw std::runtime_error.
#pragma once

#include <memory>
#include <vector>

#include "adjMatrix.h"
#include "cu_lanczos.h"
#include "device_graph.h"

class lanczosDecompMulti {
 public:
  lanczosDecompMulti(adjMatrix &A, unsigned krylov, const double *X, unsigned b, bool cuda);
  // op / time as in lanczosOptions: the Krylov spaces of L = D - A (with its stop rule, beta <= 2^-40 * 2 d_max) and answers
  // e^{-tL} x_c, or e^{tA} x_c
  lanczosDecompMulti(adjMatrix &A, unsigned krylov, const double *X, unsigned b, bool cuda, graphOperator op, double time);
  lanczosDecompMulti(const lanczosDecompMulti &) = delete;
  lanczosDecompMulti &operator=(const lanczosDecompMulti &) = delete;
  ~lanczosDecompMulti();

  unsigned get_n() const { return A.get_n(); }
  unsigned get_krylov() const { return krylov_dim; }
  unsigned get_b() const { return b; }
  const double *get_alpha() const { return alpha.data(); }     // [b][k]; 0 behind a column's k_used
  const double *get_beta() const { return beta.data(); }       // [b][k]; beta[c][k - 1] = 0
  const unsigned *k_used() const { return kused.data(); }      // [b]
  const double *x_norms() const { return xn.data(); }          // [b]
  const double *answer() const { return ans.data(); }          // [b][n] once multOutMulti ran
  double loop_ms() const { return loop_ms_; }                  // device path: the batches' loops

  friend void multOutMulti(lanczosDecompMulti &, adjMatrix &);

 private:
  adjMatrix &A;
  unsigned krylov_dim, b;
  bool cuda;
  graphOperator op = graphOperator::adjacency;
  double time = 1.0;
  std::vector<double> X, alpha, beta, xn, ans, Q;   // Q: CPU path, [b][k][n]
  std::vector<unsigned> kused;
  std::vector<char> answered;
  std::shared_ptr<deviceGraph> graph;
  double loop_ms_ = 0;

  static constexpr unsigned batch = 16;   // columns per device batch (lzx_lanczos_multi_f64)
  void decompose_column(unsigned c);      // CPU recurrence of decompose() with the breakdown stop
  void run_batch(unsigned first);         // device: the batch of columns [first, first + 16)
  void answer_batch(unsigned first);      // t_c per column, then Q_c t_c
};

void multOutMulti(lanczosDecompMulti &L, adjMatrix &A);
