// Host build of scan scoring's per-element code for the CPU test tier, compiled with g++ (tests/test_score_host.py through
// host_emulation.load_shim): score_transform on its own, and score_point over n points and K poses as k_score's threads run it — one
// (point, pose) pair at a time, a tile of kScoreTile points per "workgroup" — with the sums formed in the kernels' fixed tree (the
// butterfly over a wave's 64 lanes, the waves pairwise, then k_score_reduce over the tiles).  Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "gndt_score.hpp"
#include "shim_map.hpp"

using namespace gndt;

namespace {

// what score_wave_sum leaves in lane 0: off = 32, 16, ... 1, every lane adding its partner's value
template <typename T>
T wave_tree(const T* in) {
    T v[64], t[64];
    for (int l = 0; l < 64; ++l) v[l] = in[l];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; ++l) v[l] = t[l];
    }
    return v[0];
}

// score_block_sum of N values (N / 64 waves): the wave sums added pairwise
template <uint32_t N, typename T>
T block_tree(const T* v) {
    T s[N / 64];
    for (uint32_t w = 0; w < N / 64; ++w) s[w] = wave_tree(v + 64 * w);
    for (uint32_t w = N / 64; w > 1; w >>= 1)
        for (uint32_t i = 0; i < w / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

}  // namespace

extern "C" {

// q[i] = score_transform(T, xyz[i]) for n points of sf floats each
void sshim_transform(const double* T, const float* xyz, uint32_t sf, uint64_t n, float* q) {
    for (uint64_t i = 0; i < n; ++i) score_transform(T, xyz[i * sf], xyz[i * sf + 1], xyz[i * sf + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
}

// K poses over n points against the rows and the column index (consumer_shim's build_index).  out: K records.  For pose point_pose
// (when < K) and wherever the pointer is not null: every point's least d2 and its row (the kernel's per-point outputs), and — the
// shim's own — the number of its terms and the sum of their d2 (the thread's sums before any reduction).
int sshim_score(int nbh, const float* xyz, uint32_t sf, uint64_t n, const double* poses, uint32_t K, const ShimMap* m, uint32_t min_count,
                double cov_rel, double cov_floor, double max_d2, uint32_t point_pose, ScoreRecord* out, float* point_d2, uint32_t* point_row,
                uint32_t* point_terms, double* point_d2_sum) {
    if (nbh != kScoreDirect1 && nbh != kScoreDirect7) return 1;
    const ScoreView S{view_of(*m), m->count, m->cov};
    ScoreParams P;
    P.min_count = min_count; P.cov_rel = cov_rel; P.cov_floor = cov_floor; P.max_d2 = max_d2;
    const uint64_t tiles = (n + kScoreTile - 1) / kScoreTile;
    std::vector<ScorePartial> partial(tiles);
    for (uint32_t k = 0; k < K; ++k) {
        for (uint64_t tile = 0; tile < tiles; ++tile) {                    // k_score
            double score[kScoreTile], d2_sum[kScoreTile];
            uint32_t matched[kScoreTile], terms[kScoreTile];
            for (uint32_t t = 0; t < kScoreTile; ++t) {
                const uint64_t i = tile * kScoreTile + t;
                ScoreAcc a;
                a.score = 0.0; a.d2_sum = 0.0; a.matched = 0u; a.terms = 0u;
                if (i < n) {
                    float qx, qy, qz;
                    score_transform(poses + 12 * (size_t)k, xyz[i * sf], xyz[i * sf + 1], xyz[i * sf + 2], qx, qy, qz);
                    ScoreBest b;
                    b.d2 = (double)INFINITY; b.row = kNoRow;
                    if (nbh == kScoreDirect1) score_point<kScoreDirect1>(S, P, qx, qy, qz, a, b);
                    else score_point<kScoreDirect7>(S, P, qx, qy, qz, a, b);
                    if (k == point_pose) {
                        if (point_d2) point_d2[i] = (float)b.d2;
                        if (point_row) point_row[i] = b.row;
                        if (point_terms) point_terms[i] = a.terms;
                        if (point_d2_sum) point_d2_sum[i] = a.d2_sum;
                    }
                }
                score[t] = a.score; d2_sum[t] = a.d2_sum; matched[t] = a.matched; terms[t] = a.terms;
            }
            partial[tile].score = block_tree<kScoreTile>(score); partial[tile].d2_sum = block_tree<kScoreTile>(d2_sum);
            partial[tile].matched = block_tree<kScoreTile>(matched); partial[tile].terms = block_tree<kScoreTile>(terms);
        }
        std::vector<double> score(kScoreReduceBlock), d2_sum(kScoreReduceBlock);          // k_score_reduce
        std::vector<uint64_t> matched(kScoreReduceBlock), terms(kScoreReduceBlock);
        for (uint32_t t = 0; t < kScoreReduceBlock; ++t) {
            score[t] = 0.0; d2_sum[t] = 0.0; matched[t] = 0; terms[t] = 0;
            for (uint64_t j = t; j < tiles; j += kScoreReduceBlock) {
                score[t] += partial[j].score; d2_sum[t] += partial[j].d2_sum; matched[t] += partial[j].matched; terms[t] += partial[j].terms;
            }
        }
        out[k].score = block_tree<kScoreReduceBlock>(score.data()); out[k].d2_sum = block_tree<kScoreReduceBlock>(d2_sum.data());
        out[k].matched = block_tree<kScoreReduceBlock>(matched.data()); out[k].terms = block_tree<kScoreReduceBlock>(terms.data());
    }
    return 0;
}

}  // extern "C"
