// Nearest-word search over an embedding table (coco/glove.py: closest, closest_batch) in fp32, D = 300 fixed.
//   score(q, v) = sqnorm[v] - 2 q.w_v   ranks the words of a query (|q|^2 is the same for every word of a query);
//   the dot product is ONE fixed fmaf chain per (query, word) pair on v_mfma_f32_32x32x2_f32, so the score of a pair -- and
//   with the lowest-index tie rule the winner -- does not depend on the tile, the split or the batch the pair lands in.
//   The reported distance is recomputed directly as sqrt(sum (q - w)^2): the score form cancels when q ~ w.
#pragma once
#include "common.h"

enum {
    NNW_DIM = 300,           // embedding width (GloVe-840B), compile-time
    NNW_TQ = 256,            // query rows per workgroup: 8 waves x 32 rows, kept in registers as MFMA A operands
    NNW_TV = 32,             // words per vocabulary tile (one 32-column MFMA tile per wave per LDS buffer)
    NNW_MAX_SPLITS = 512,    // vocabulary splits: grid = (query blocks) x (splits)
    NNW_MAX_DISTS = 8,       // queries of one nn_words_dists call
};

// Number of vocabulary splits for a shape: a function of the shape alone (never of the device), so that workspace sizes and
// launch shapes are reproducible: max(1, min(NNW_MAX_SPLITS, tiles, 1024 / query blocks)) -- at most 1024 workgroups in all,
// never more splits than tiles (include/mmvae_hip.h states the rule for callers).
int nn_words_splits(int n_queries, long long n_words);
size_t nn_words_workspace_bytes(int n_queries, long long n_words);

int launch_nn_words_norms(const float* table, long long n_words, float* sqnorm, hipStream_t s);
// ws: nn_words_workspace_bytes(n_queries, n_words) bytes; index [n_queries] int64, dist [n_queries] float
int launch_nn_words_nearest(const float* queries, int n_queries, const float* table, const float* sqnorm, long long n_words,
                            void* ws, long long* index, float* dist, hipStream_t s);
// dist [n_queries][n_words], n_queries <= NNW_MAX_DISTS
int launch_nn_words_dists(const float* queries, int n_queries, const float* table, long long n_words, float* dist, hipStream_t s);
