// gndt_shortcut.hpp — route shortcutting (include/gndt.h "route shortcutting"): K routes of slope rows (gndt_plan_routes' layout) are
// string-pulled into any-angle waypoints.  A link a -> b is the path walk (gndt_walk.hpp: walk_step / walk_enter over ray_begin /
// ray_next's column sequence) of the straight line between the two rows' column centres, started standing on row a, and holds iff it
// ends DONE on row b.  Per route the anchors advance greedily: the candidates behind the anchor in groups of 64 counted from it, the
// farthest group first, the largest holding candidate of the first group that has one; none: the route's own next row, untested.
//   k_shortcut_routes   one route a wavefront (like a query in gndt_plan.hpp), the 64 lanes the 64 candidates of a group: every lane
//                       walks its link, a ballot and its highest bit choose the anchor, then the whole wavefront walks the chosen link
//                       once more in step (the same addresses in every lane) and its leader writes the slopes, so that the sums stay
//                       one thread's sequential arithmetic.  The anchor loop is the dependent chain.
// Everything up to the kernel is callable on the host, so that the CPU test tier runs the kernel's own code lane after lane
// (tests/shortcut_shim.cpp, ShortcutWaveHost).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gndt_walk.hpp"

namespace gndt {

constexpr int kShortcutOk = 0, kShortcutEmpty = 1, kShortcutBadRoute = 2, kShortcutLimit = 3;      // GNDT_SHORTCUT_*
constexpr uint32_t kShortcutLanes = 64;
constexpr uint32_t kShortcutDefaultWindow = 64u, kShortcutMaxWindow = 256u;
constexpr uint32_t kShortcutDefaultLinks = 1u << 20, kShortcutMaxLinks = 1u << 24;

struct ShortcutRule {            // gndt_shortcut_params with its defaults resolved
    uint32_t window, max_links;
    WalkRule walk;               // checks and min_hops (start_mode and max_steps are not read: a link has at most `window` steps)
};

struct ShortcutInfo {            // gndt_shortcut_info
    int32_t status;
    uint32_t length_in, waypoints, path_slopes;
    uint32_t links_tested, fallback_links;
    float cost_in, cost_out;
    uint32_t hops_min;
    uint32_t reserved[3];
};

struct ShortcutSink {            // where an accepted link's slopes go: the route's path so far
    uint32_t* path;              // [cap] or null with 0
    uint32_t cap, n;             // n: slopes so far, written or not
    double cost;                 // the sum of cost_travel over consecutive slopes, in order
    uint32_t hops_min;
    bool write;                  // this lane stores (the wavefront's leader)
};

// The centre of column s on an axis (no index 0): what map2d._column_centre computes, rounded to fp32 once
GNDT_HD float shortcut_centre(float o, float grid_len, int s) {
    const double a = (double)(s < 0 ? -s : s) - 0.5;
    return (float)((double)o + (s > 0 ? a : -a) * (double)grid_len);
}

GNDT_HD void shortcut_append(const CostView& V, ShortcutSink& s, uint32_t from, uint32_t t) {
    s.cost += (double)cost_travel(V.mean + 3 * (size_t)from, V.mean + 3 * (size_t)t);
    if (s.write && s.n < s.cap) s.path[s.n] = t;
    s.n += 1u;
}

// Link(a, b) of include/gndt.h.  OUT: the link is known to hold and its slopes behind a go into the sink.
template <bool OUT>
GNDT_HD bool shortcut_link(const QueryView& Q, const Robot& R, const ShortcutRule& P, const uint32_t* hops, uint32_t num_rows, uint32_t a,
                           uint32_t b, ShortcutSink* sink) {
    const CostView& V = Q.V;
    if (a >= num_rows || b >= num_rows || !row_has_slope(V, a) || !row_has_slope(V, b)) return false;
    const int ax = V.sx[a], ay = V.sy[a], bx = V.sx[b], by = V.sy[b];
    const float pax = shortcut_centre(Q.ox, Q.grid_len, ax), pay = shortcut_centre(Q.oy, Q.grid_len, ay);
    const float pbx = shortcut_centre(Q.ox, Q.grid_len, bx), pby = shortcut_centre(Q.oy, Q.grid_len, by);
    const float z = V.mean[3 * (size_t)a + 2];
    const PointKey ka = point_key(pax, pay, z, Q.ox, Q.oy, Q.oz, Q.grid_len, Q.z_len);
    const PointKey kb = point_key(pbx, pby, z, Q.ox, Q.oy, Q.oz, Q.grid_len, Q.z_len);
    if (!ka.ok || !kb.ok || ka.sx != ax || ka.sy != ay || kb.sx != bx || kb.sy != by) return false;
    const int dx = ray_lin(bx) - ray_lin(ax), dy = ray_lin(by) - ray_lin(ay);
    if ((uint32_t)(dx < 0 ? -dx : dx) + (uint32_t)(dy < 0 ? -dy : dy) > P.window) return false;
    RayGrid G;
    G.ox = Q.ox; G.oy = Q.oy; G.oz = Q.oz; G.grid_len = Q.grid_len; G.z_len = Q.z_len;
    G.rx = G.ry = G.rz = 0.f; G.max_range = 0.f; G.end_margin = 0.f;
    RayWalk w;
    if (!ray_begin(G, pax, pay, z, pbx, pby, z, w)) return false;
    WalkInfo o;
    o.end_row = kNoRow; o.rough_max = 0.f; o.hops_min = kClrBeyond;
    const WalkTable none{nullptr, nullptr};
    uint32_t q = a, c = ctab_find(V, ax, ay), stood = 0u;
    int cx = ax, cy = ay;
    bool ok = walk_enter(V, R, P.walk, hops, q, c, stood++, nullptr, 0u, o) == kWalkDone;
    RayColumn rc;
    ray_next(G, w, rc);                                  // (a's column)
    while (ok && ray_next(G, w, rc)) {
        const uint32_t k = rc.sx == cx ? (rc.sy < cy ? 0u : 1u) : (rc.sx > cx ? 2u : 3u);
        float dz;
        const uint32_t t = walk_step<false>(V, R, none, q, k, rc.sx, rc.sy, c, dz);
        if (t == kNoRow) { ok = false; break; }
        if (OUT) shortcut_append(V, *sink, q, t);
        q = t; cx = rc.sx; cy = rc.sy;
        ok = walk_enter(V, R, P.walk, hops, q, c, stood++, nullptr, 0u, o) == kWalkDone;
    }
    if (OUT) sink->hops_min = o.hops_min < sink->hops_min ? o.hops_min : sink->hops_min;
    return ok && q == b;
}

// A fallback link: the route's own next row, untested
GNDT_HD void shortcut_fallback(const CostView& V, const uint32_t* hops, ShortcutSink& s, uint32_t from, uint32_t t) {
    shortcut_append(V, s, from, t);
    if (hops) { const uint32_t hp = hops[t]; s.hops_min = hp < s.hops_min ? hp : s.hops_min; }
}

// The group choice: the largest candidate of the group whose link holds, as its offset in the group (mask != 0)
GNDT_HD uint32_t shortcut_pick(uint64_t mask) { return 63u - (uint32_t)__builtin_clzll(mask); }

struct ShortcutWaveHost {        // the wavefront's collectives, lane after lane
    template <typename F> static uint64_t ballot(F f) {
        uint64_t m = 0;
        for (uint32_t l = 0; l < kShortcutLanes; ++l) m |= f(l) ? 1ull << l : 0ull;
        return m;
    }
    template <typename F> static void each(F f) { for (uint32_t l = 0; l < kShortcutLanes; ++l) f(l); }
    template <typename F> static void add_in_order(double& acc, uint32_t count, F term) {
        for (uint32_t l = 0; l < count; ++l) acc += (double)term(l);
    }
    static bool leader() { return true; }
};

// One route: r[n] its rows (n from the caller's lengths), wp[wp_cap] the anchors, path[path_cap] (or null with 0) the slopes stood on.
template <typename W>
GNDT_HD void shortcut_route(const QueryView& Q, const Robot& R, const ShortcutRule& P, const uint32_t* hops, uint32_t num_rows, const uint32_t* r,
                            uint32_t n, uint32_t route_cap, uint32_t* wp, uint32_t wp_cap, uint32_t* path, uint32_t path_cap, ShortcutInfo& o) {
    const CostView& V = Q.V;
    o.status = kShortcutOk; o.length_in = n; o.waypoints = 0u; o.path_slopes = 0u; o.links_tested = 0u; o.fallback_links = 0u;
    o.cost_in = 0.f; o.cost_out = 0.f; o.hops_min = kClrBeyond;
    o.reserved[0] = o.reserved[1] = o.reserved[2] = 0u;
    const bool leader = W::leader();
    uint32_t wn = 0u;
    ShortcutSink s{path, path_cap, 0u, 0.0, kClrBeyond, leader};
    if (n == 0u) o.status = kShortcutEmpty;
    else if (n > route_cap) o.status = kShortcutBadRoute;
    else
        for (uint32_t i = 0; i < n; i += kShortcutLanes)
            if (W::ballot([&](uint32_t lane) {
                    const uint32_t row = i + lane < n ? r[i + lane] : 0u;
                    return i + lane < n && (row >= num_rows || !row_has_slope(V, row));
                }))
                o.status = kShortcutBadRoute;
    if (o.status == kShortcutOk) {
        double cost_in = 0.0;
        for (uint32_t i = 0; i + 1u < n; i += kShortcutLanes) {
            const uint32_t count = n - 1u - i < kShortcutLanes ? n - 1u - i : kShortcutLanes;
            W::add_in_order(cost_in, count, [&](uint32_t lane) {
                return lane < count ? cost_travel(V.mean + 3 * (size_t)r[i + lane], V.mean + 3 * (size_t)r[i + lane + 1u]) : 0.f;
            });
        }
        o.cost_in = (float)cost_in;
        auto anchor = [&](uint32_t row) {
            if (leader && wn < wp_cap) wp[wn] = row;
            wn += 1u;
        };
        anchor(r[0]);
        if (leader && path_cap) path[0] = r[0];
        s.n = 1u;
        if (hops) s.hops_min = hops[r[0]];
        uint32_t a = 0u;
        while (a + 1u < n) {
            const uint32_t cand = n - 1u - a < P.window ? n - 1u - a : P.window;
            uint32_t next = 0u;
            bool limit = false;
            for (uint32_t g = (cand + kShortcutLanes - 1u) / kShortcutLanes; g-- > 0u && !next;) {
                const uint32_t base = a + g * kShortcutLanes + 1u;
                const uint32_t size = cand - g * kShortcutLanes < kShortcutLanes ? cand - g * kShortcutLanes : kShortcutLanes;
                if (o.links_tested + size > P.max_links) { limit = true; break; }
                o.links_tested += size;
                const uint32_t ra = r[a];
                const uint64_t holds = W::ballot([&](uint32_t lane) {
                    return lane < size && shortcut_link<false>(Q, R, P, hops, num_rows, ra, r[base + lane], nullptr);
                });
                if (holds) next = base + shortcut_pick(holds);
            }
            if (limit) {                                 // the rest of the route as it came
                o.status = kShortcutLimit;
                for (uint32_t i = a + 1u; i < n; ++i) {
                    shortcut_fallback(V, hops, s, r[i - 1u], r[i]);
                    anchor(r[i]);
                    o.fallback_links += 1u;
                }
                break;
            }
            if (next) {
                shortcut_link<true>(Q, R, P, hops, num_rows, r[a], r[next], &s);
            } else {
                next = a + 1u;
                shortcut_fallback(V, hops, s, r[a], r[next]);
                o.fallback_links += 1u;
            }
            anchor(r[next]);
            a = next;
        }
    }
    o.waypoints = wn;
    o.path_slopes = s.n;
    o.cost_out = (float)s.cost;
    o.hops_min = s.hops_min;
    const uint32_t wf = wn < wp_cap ? wn : wp_cap, pf = s.n < path_cap ? s.n : path_cap;
    W::each([&](uint32_t lane) {
        for (uint32_t i = wf + lane; i < wp_cap; i += kShortcutLanes) wp[i] = kNoRow;
        for (uint32_t i = pf + lane; i < path_cap; i += kShortcutLanes) path[i] = kNoRow;
    });
}

}  // namespace gndt

#if defined(__HIPCC__)
namespace gndt {

struct ShortcutWaveDevice {
    template <typename F> static __device__ __forceinline__ uint64_t ballot(F f) { return __ballot(f((uint32_t)(threadIdx.x & 63u)) ? 1 : 0); }
    template <typename F> static __device__ __forceinline__ void each(F f) { f((uint32_t)(threadIdx.x & 63u)); }
    // every lane's term once, then added lane after lane by all of them: the sum is one thread's sequential fp64 arithmetic
    template <typename F> static __device__ __forceinline__ void add_in_order(double& acc, uint32_t count, F term) {
        const float mine = term((uint32_t)(threadIdx.x & 63u));
        for (uint32_t l = 0; l < count; ++l) acc += (double)__shfl(mine, (int)l, 64);
    }
    static __device__ __forceinline__ bool leader() { return (threadIdx.x & 63u) == 0u; }
};

// One route a wavefront, kShortcutWaves wavefronts a workgroup that share nothing (no LDS, no barrier); grid-stride over the routes.
// info: three 16-byte stores a route, by the wavefront's leader.
constexpr int kShortcutWaves = 4, kShortcutThreads = kShortcutWaves * 64, kShortcutMaxBlocks = 1024;
static __global__ void __launch_bounds__(kShortcutThreads) k_shortcut_routes(QueryView Q, Robot R, ShortcutRule P, uint32_t num_rows,
                                                                            const uint32_t* __restrict__ hops, const uint32_t* __restrict__ routes,
                                                                            uint64_t K, uint32_t route_cap, const char* __restrict__ lengths,
                                                                            uint64_t length_stride, uint32_t* __restrict__ wp, uint32_t wp_cap,
                                                                            uint32_t* __restrict__ path, uint32_t path_cap,
                                                                            ShortcutInfo* __restrict__ info) {
    const uint64_t waves = (uint64_t)gridDim.x * kShortcutWaves;
    for (uint64_t k = (uint64_t)blockIdx.x * kShortcutWaves + (threadIdx.x >> 6); k < K; k += waves) {
        const uint32_t n = *reinterpret_cast<const uint32_t*>(lengths + k * length_stride);
        ShortcutInfo o;
        shortcut_route<ShortcutWaveDevice>(Q, R, P, hops, num_rows, routes + k * route_cap, n, route_cap, wp + k * wp_cap, wp_cap,
                                           path ? path + k * path_cap : nullptr, path_cap, o);
        if ((threadIdx.x & 63u) == 0u) {
            uint4* out = reinterpret_cast<uint4*>(info + k);
            out[0] = make_uint4((uint32_t)o.status, o.length_in, o.waypoints, o.path_slopes);
            out[1] = make_uint4(o.links_tested, o.fallback_links, float_bits(o.cost_in), float_bits(o.cost_out));
            out[2] = make_uint4(o.hops_min, 0u, 0u, 0u);
        }
    }
}

}  // namespace gndt
#endif  // __HIPCC__
