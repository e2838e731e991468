// The epilogue of the vocabulary-scoring units (forward_vocab.hip, gmm_vocab.hip, full_vocab.hip) over
// score[n_utts][W].  Included INSIDE the unit's `namespace sapr { namespace {`, after viterbi_shared.h (kBlock,
// neg_inf).
#pragma once

// One lane per utterance over its row of W scores: the arg-max word of decoder.py:42-47 (first strict maximum in model
// order from -inf; -1 when no score beats -inf) and the posterior over the words under a uniform prior,
// exp(score - logsumexp_w score), evaluated as exp(score - max) / sum_w exp(score - max): the subtraction of a
// rounded logsumexp of magnitude 10^4 would cost the posteriors three digits.  A row whose maximum is -inf gives NaN
// (exp(-inf + inf)), a NaN score makes the row's sum NaN: nothing is repaired.
__global__ __launch_bounds__(kBlock) void vocab_epilogue_kernel(int64_t n_utts, int32_t W,
                                                                    const double *__restrict__ score,
                                                                    int32_t *__restrict__ best_word,
                                                                    double *__restrict__ word_post) {
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (u >= n_utts) return;
  const double *__restrict__ row = score + u * W;
  int bw = -1;
  double bs = neg_inf();
  for (int w = 0; w < W; ++w) {
    const double sc = row[w];
    if (sc > bs) {
      bs = sc;
      bw = w;
    }
  }
  if (best_word) best_word[u] = bw;
  if (!word_post) return;
  double den = 0.0;
  for (int w = 0; w < W; ++w) den += exp(row[w] - bs);
  for (int w = 0; w < W; ++w) word_post[u * W + w] = exp(row[w] - bs) / den;
}

inline int launch_vocab_epilogue(int64_t n_utts, int32_t W, const double *score, int32_t *best_word,
                                 double *word_post, hipStream_t stream) {
  SAPR_LAUNCH(vocab_epilogue_kernel, dim3(static_cast<unsigned>((n_utts + kBlock - 1) / kBlock)), dim3(kBlock), 0,
              stream, n_utts, W, score, best_word, word_post);
  SAPR_HIP_TRY(hipGetLastError());
  return 0;
}
