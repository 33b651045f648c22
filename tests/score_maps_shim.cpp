// Host build of map-to-map scoring's per-element code for the CPU test tier, compiled with g++ (tests/test_score_maps_host.py through
// host_emulation.load_shim): score_maps_row over the source rows and K poses as k_score_maps / k_score_maps_derivs' threads run it —
// one (source row, pose) pair at a time, a tile of kScoreTile rows per "workgroup" — with all 4 + 27 sums formed in the kernels' fixed
// tree (the butterfly over a wave's 64 lanes, the waves pairwise, then the tiles as the score's reduce kernels add them).
// Test infrastructure only.
#include <stdint.h>

#include <vector>

#include "gndt_score_maps.hpp"
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

// N values (N / 64 waves): the wave sums added pairwise
template <typename T>
T block_tree(const T* v, uint32_t N) {
    std::vector<T> s(N / 64);
    for (uint32_t w = 0; w < N / 64; ++w) s[w] = wave_tree(v + 64 * w);
    for (uint32_t w = N / 64; w > 1; w >>= 1)
        for (uint32_t i = 0; i < w / 2; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

}  // namespace

extern "C" {

// K poses over the rows of the source map `src` (its count, mean, cov and flags) against the destination's rows and column index
// (consumer_shim's build_index).  out: K records of 31 eight-byte fields (gndt_pose_derivs; with derivs == 0 the 27 values stay 0:
// k_score_maps' record in its first four fields).  node_d2 / node_row (may be null): the per-node outputs of pose node_pose.
// node_vals (may be null): the 27 values of every source row at that pose, before any reduction.
int mshim_score_maps(int nbh, int derivs, const ShimMap* src, const double* poses, uint32_t K, const ShimMap* dst, uint32_t min_count,
                     double cov_rel, double cov_floor, double max_d2, ScoreDerivRecord* out, uint32_t node_pose, float* node_d2,
                     uint32_t* node_row, double* node_vals) {
    if (nbh != kScoreDirect1 && nbh != kScoreDirect7) return 1;
    const ScoreView D{view_of(*dst), dst->count, dst->cov};
    const MapsSource M{src->count, src->mean, src->cov, src->flags};
    const uint64_t n = src->n;
    ScoreParams P;
    P.min_count = min_count; P.cov_rel = cov_rel; P.cov_floor = cov_floor; P.max_d2 = max_d2;
    const uint64_t tiles = (n + kScoreTile - 1) / kScoreTile;
    std::vector<ScoreDerivPartial> partial(tiles);
    for (uint32_t k = 0; k < K; ++k) {
        const double* T = poses + 12 * (size_t)k;
        for (uint64_t tile = 0; tile < tiles; ++tile) {                    // k_score_maps / k_score_maps_derivs
            std::vector<double> v((size_t)kDerivDoubles * kScoreTile);
            uint32_t matched[kScoreTile], terms[kScoreTile];
            for (uint32_t t = 0; t < kScoreTile; ++t) {
                const uint64_t i = tile * kScoreTile + t;
                ScoreAcc a;
                a.score = 0.0; a.d2_sum = 0.0; a.matched = 0u; a.terms = 0u;
                double o[kDerivValues];
                for (int j = 0; j < kDerivValues; ++j) o[j] = 0.0;
                if (i < n) {
                    ScoreBest b;
                    b.d2 = (double)INFINITY; b.row = kNoRow;
                    bool counted;
                    if (nbh == kScoreDirect1)
                        counted = derivs ? score_maps_row<kScoreDirect1, true>(D, P, M, i, T, a, b, o)
                                         : score_maps_row<kScoreDirect1, false>(D, P, M, i, T, a, b, nullptr);
                    else
                        counted = derivs ? score_maps_row<kScoreDirect7, true>(D, P, M, i, T, a, b, o)
                                         : score_maps_row<kScoreDirect7, false>(D, P, M, i, T, a, b, nullptr);
                    if (k == node_pose) {
                        if (node_d2) node_d2[i] = counted ? (float)b.d2 : NAN;
                        if (node_row) node_row[i] = b.row;
                        if (node_vals)
                            for (int j = 0; j < kDerivValues; ++j) node_vals[i * kDerivValues + j] = o[j];
                    }
                }
                v[0 * kScoreTile + t] = a.score; v[1 * kScoreTile + t] = a.d2_sum;
                for (int j = 0; j < kDerivValues; ++j) v[(size_t)(2 + j) * kScoreTile + t] = o[j];
                matched[t] = a.matched; terms[t] = a.terms;
            }
            for (int j = 0; j < kDerivDoubles; ++j) partial[tile].v[j] = block_tree(v.data() + (size_t)j * kScoreTile, kScoreTile);
            partial[tile].matched = block_tree(matched, kScoreTile); partial[tile].terms = block_tree(terms, kScoreTile);
        }
        std::vector<double> v((size_t)kDerivDoubles * kScoreReduceBlock, 0.0);          // the score's reduce kernels
        std::vector<uint64_t> matched(kScoreReduceBlock, 0), terms(kScoreReduceBlock, 0);
        for (uint32_t t = 0; t < kScoreReduceBlock; ++t)
            for (uint64_t j = t; j < tiles; j += kScoreReduceBlock) {
                for (int f = 0; f < kDerivDoubles; ++f) v[(size_t)f * kScoreReduceBlock + t] += partial[j].v[f];
                matched[t] += partial[j].matched; terms[t] += partial[j].terms;
            }
        double r[kDerivDoubles];
        for (int f = 0; f < kDerivDoubles; ++f) r[f] = block_tree(v.data() + (size_t)f * kScoreReduceBlock, kScoreReduceBlock);
        out[k].score = r[0]; out[k].d2_sum = r[1];
        out[k].matched = block_tree(matched.data(), kScoreReduceBlock); out[k].terms = block_tree(terms.data(), kScoreReduceBlock);
        for (int j = 0; j < 6; ++j) out[k].g[j] = r[2 + j];
        for (int j = 0; j < 21; ++j) out[k].H[j] = r[8 + j];
    }
    return 0;
}

// n points q against the rows `rows` of the map: d2 of score_maps_pair with Sigma = 0 (pair_d2) and of score_node (node_d2), and
// whether each counts
void mshim_pair_zero_sigma(const float* q, const uint32_t* rows, uint64_t n, const ShimMap* m, uint32_t min_count, double cov_rel,
                           double cov_floor, double max_d2, double* pair_d2, double* node_d2, uint8_t* pair_ok, uint8_t* node_ok) {
    const ScoreView D{view_of(*m), m->count, m->cov};
    ScoreParams P;
    P.min_count = min_count; P.cov_rel = cov_rel; P.cov_floor = cov_floor; P.max_d2 = max_d2;
    for (uint64_t i = 0; i < n; ++i) {
        MapsNode m{};
        m.qx = q[3 * i]; m.qy = q[3 * i + 1]; m.qz = q[3 * i + 2];
        ScoreTerm a{}, b{};
        pair_ok[i] = score_maps_pair(D, P, m, rows[i], a);
        node_ok[i] = score_node(D, P, rows[i], m.qx, m.qy, m.qz, b);
        pair_d2[i] = a.d2; node_d2[i] = b.d2;
    }
}

}  // extern "C"
