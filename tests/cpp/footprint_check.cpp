// Stand-alone check of the footprint poses' per-pose code (grid_ndt_amd/csrc/gndt_footprint.hpp) under the sanitizers: random cell
// tables drawn here (one to three levels a column, a few rows without a slope, random counts and scatters), the column index filled
// the way the library fills it, then poses of every footprint size from n = 1 to n = 15 through foot_pose lane after lane, with and
// without rows and a band.  Host code only.  Prints "ok <poses> <supports>"; any finding of the sanitizers aborts.
// Built and run by tests/test_footprint_host.py:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I grid_ndt_amd/csrc
#include <stdint.h>
#include <stdio.h>

#include <memory>
#include <vector>

#include "gndt_footprint.hpp"

using namespace gndt;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
static double uni() { return rnd() / 2147483648.0; }

int main() {
    uint64_t poses = 0, supports = 0;
    auto w = std::make_unique<FootWaveHost>();
    for (int table = 0; table < 40; ++table) {
        const int side = 6 + (int)(rnd() % 20u);
        std::vector<int32_t> sx, sy, sz;
        std::vector<float> mean, cov;
        std::vector<uint32_t> flags, count, ncol;
        for (int ix = -side / 2; ix < side / 2; ++ix)
            for (int iy = -side / 2; iy < side / 2; ++iy) {
                if (uni() > 0.85) continue;
                const uint32_t levels = 1u + rnd() % 3u;
                for (uint32_t l = 0; l < levels; ++l) {
                    sx.push_back(ix >= 0 ? ix + 1 : ix); sy.push_back(iy >= 0 ? iy + 1 : iy); sz.push_back((int)l * 4 + 1);
                    mean.push_back((float)(ix * 0.5 + uni() * 0.5)); mean.push_back((float)(iy * 0.5 + uni() * 0.5));
                    mean.push_back((float)(l * 1.0 + uni() * 0.2));
                    const double a = uni() * 0.1, b = uni() * 0.1, c = uni() * 0.01;
                    const uint32_t n = 3u + rnd() % 100u;
                    const float S[6] = {(float)(n * a * a), (float)(n * a * b * 0.5), 0.f, (float)(n * b * b), 0.f, (float)(n * c * c)};
                    cov.insert(cov.end(), S, S + 6);
                    count.push_back(n);
                    flags.push_back(uni() < 0.9 ? 3u : 1u);
                    ncol.push_back(l == 0 ? levels : 0u);
                }
            }
        const uint32_t rows = (uint32_t)sx.size();
        if (!rows) continue;
        uint32_t slots = 64;
        while (slots < 2 * rows) slots <<= 1;
        std::vector<uint64_t> key(slots, kEmptyKey);
        std::vector<uint32_t> val(slots, 0u);
        for (uint32_t r = 0; r < rows; ++r) {
            if (!ncol[r]) continue;
            uint32_t s = (uint32_t)mix64(column_pack(sx[r], sy[r])) & (slots - 1);
            while (key[s] != kEmptyKey) s = (s + 1) & (slots - 1);
            key[s] = column_pack(sx[r], sy[r]); val[s] = r;
        }
        ScoreView S{};
        CostView& V = S.Q.V;
        V.sx = sx.data(); V.sy = sy.data(); V.sz = sz.data(); V.mean = mean.data(); V.flags = flags.data(); V.row_ncol = ncol.data();
        V.ctab_key = key.data(); V.ctab_val = val.data(); V.ctab_mask = slots - 1;
        S.Q.ox = S.Q.oy = S.Q.oz = 0.f; S.Q.grid_len = 0.5f; S.Q.z_len = 0.25f;
        S.count = count.data(); S.cov = cov.data();
        const Robot R{0.25f, 0.15f, 100.f, 30.f};
        for (uint32_t n = 1; n <= kFootMaxN; ++n) {
            const double half = n * 0.5 * 0.6;
            FootRule F{half * half, half * half * 0.5, 0.8660254037844387, 0.5, n % 2 ? 0.f : 0.3f, 1.5f, R.reach, 3u, n % 2u, n};
            for (int k = 0; k < 6; ++k) {
                const uint32_t r = rnd() % rows;
                float pose[5] = {mean[3 * r] + (float)(uni() - 0.5), mean[3 * r + 1] + (float)(uni() - 0.5), mean[3 * r + 2] + (float)(uni() - 0.5),
                                 (float)(uni() - 0.5), (float)(uni() - 0.5)};
                if (k == 5) pose[0] += 100.f;                // off the map
                const uint32_t cap = k % 3 == 0 ? 0u : k % 3 == 1 ? 5u : 1000u;
                std::vector<uint32_t> out(cap);
                FootInfo o;
                foot_pose(S, R, F, pose, cap ? out.data() : nullptr, cap, *w, o);
                if (o.status == kFootOk || o.status == kFootSparse) {
                    if ((uint32_t)o.cells != (uint32_t)o.support + o.gaps + o.unknown) { printf("counts differ\n"); return 1; }
                    for (uint32_t i = 0; i < cap; ++i)
                        if ((i < o.support) != (out[i] != kNoRow) || (out[i] != kNoRow && out[i] >= rows)) { printf("rows differ\n"); return 1; }
                    supports += o.support;
                }
                poses += 1;
            }
        }
    }
    printf("ok %llu %llu\n", (unsigned long long)poses, (unsigned long long)supports);
    return 0;
}
