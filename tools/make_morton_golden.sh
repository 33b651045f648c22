#!/bin/bash
# Regenerates tests/golden/morton_known_answers.csv from the REFERENCE's own key helpers, compiled where they lie:
#   countMorton(a, b)           include/Stopwatch.h:116-147  (with decToBinStr2 :39-47, binToDec :102-110, intToString :59-64)
#   mortonToXY(a, b, morton)    include/Stopwatch.h:171-189  (with strToInt :20-25)
#
#   GNDT_REFERENCE=<reference tree> tools/make_morton_golden.sh [out.csv]      (default: tests/golden/morton_known_answers.csv)
#
# This is the one piece of the path the reference pins by itself and that compiles in this image: the header needs
# nothing but the standard library for these functions.  Its line 9 includes <boost/format.hpp> without using it in them; Boost
# is not installed here, so the include is satisfied by an EMPTY file in a temporary directory that is deleted again (nothing of
# Boost is restated; VERDICT r5 item 7 asks for exactly this recipe).  The caller below is this repo's; nothing of the reference
# is copied, and only the CSV (data: inputs and the reference's answers) is committed and travels to the GPU box.
# tests/test_oracle_golden.py::test_golden_file_regenerates re-runs this script when GNDT_REFERENCE is set and diffs; without it,
# the test restates this script's rows and answers them with the oracle.
set -euo pipefail
ref=${GNDT_REFERENCE:?set GNDT_REFERENCE to the reference tree}
root=$(cd "$(dirname "$0")/.." && pwd)
out=${1:-$root/tests/golden/morton_known_answers.csv}
[ -f "$ref/include/Stopwatch.h" ] || { echo "no reference at $ref: the committed CSV stays as it is" >&2; exit 3; }
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/shim/boost"
: > "$tmp/shim/boost/format.hpp"
cat > "$tmp/gen.cpp" <<'EOF'
// caller of the reference helpers (this repo's code; the header forgets <vector> and <algorithm>)
#include <vector>
#include <algorithm>
#include <cstdio>
#include <set>
#include <utility>
#include "Stopwatch.h"
int main() {
    std::vector<std::pair<int, int>> rows;
    std::set<std::pair<int, int>> seen;
    auto add = [&](long a, long b) {
        if (a < 0 || b < 0 || a > 70000 || b > 70000) return;
        const std::pair<int, int> p((int)a, (int)b);
        if (seen.insert(p).second) rows.push_back(p);
    };
    // (1) the rows SURVEY Appendix B lists, in its order (row 5,7 -> 55 is the header's worked example, Stopwatch.h:112-115)
    const int listed[][2] = {{1,1},{1,2},{2,1},{2,2},{3,5},{5,3},{5,7},{7,5},{8,1},{1,8},{16,16},{100,1},{1,100},{100,200},{255,255},
                             {256,256},{1000,1},{1000,1000},{4095,4095},{32767,32767},{1,32768},{32768,1},{32768,32768},{65535,65535},
                             {65536,1},{1,65536},{0,0},{0,1},{1,0}};
    for (auto& r : listed) add(r[0], r[1]);
    // (2) every pair of 1 .. 64
    for (int a = 1; a <= 64; ++a) for (int b = 1; b <= 64; ++b) add(a, b);
    // (3) powers of two and their neighbours against each other and against 1
    std::vector<long> edge;
    for (int k = 0; k <= 16; ++k) for (int d = -1; d <= 1; ++d) edge.push_back((1L << k) + d);
    // (4) the uniqueness / decode limits (SURVEY Appendix B: decode breaks above 32 767, keys wrap above 65 535)
    for (long v : {32766L, 32767L, 32768L, 32769L, 65534L, 65535L, 65536L, 65537L, 40000L, 70000L}) edge.push_back(v);
    for (long a : edge) { add(a, 1); add(1, a); add(a, a); }
    for (size_t i = 0; i < edge.size(); ++i) for (size_t j = 0; j < edge.size(); j += 3) add(edge[i], edge[(i + j) % edge.size()]);
    for (auto& r : rows) {
        const std::string m = countMorton(r.first, r.second);
        int da = 0, db = 0;
        mortonToXY(da, db, strToInt(m));
        std::printf("%d,%d,%s,%d,%d\n", r.first, r.second, m.c_str(), da, db);
    }
    return 0;
}
EOF
g++ -std=c++11 -O1 -w -I "$tmp/shim" -I "$ref/include" "$tmp/gen.cpp" -o "$tmp/gen"
{
    echo "# countMorton(a,b) and mortonToXY(strToInt(.)) as answered by the reference's own helpers"
    echo "# (include/Stopwatch.h:116-147, 171-189), compiled as-is by tools/make_morton_golden.sh — SURVEY.md Appendix B."
    echo "# Row \"5,7,55,5,7\" is also the header's worked example (Stopwatch.h:112-115, 166-170)."
    echo "# a,b,countMorton,decoded_a,decoded_b"
    "$tmp/gen"
} > "$tmp/out.csv"
mv "$tmp/out.csv" "$out"
echo "$(grep -vc '^#' "$out") rows -> $out" >&2
