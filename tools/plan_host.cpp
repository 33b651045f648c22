// plan_host.cpp — the HOST planner's side of tools/measure_plan.py: gndt_compat::AstarPlanar::findRoute in the lazy mode (the consumers
// served from the exported rows, no containers) for a list of starts on one map, each on a fresh map as the reference's callback has it
// (create2DMap -> computeCost -> findRoute, receiver.cpp:160-176), timed for the route alone; the gndt_export_host the host planner
// needs is timed by create2DMap (TwoDmap::timing).  Built like tools/host_path.cpp.
//   plan_host <cloud.f32> <n> <grid_len> <z_len> <interval> <demand> <gx> <gy> <gz> <radius> <starts.f32> <K>
// prints ONE JSON object (milliseconds).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gndt_compat.hpp"

using namespace gndt_compat;
using Clock = std::chrono::steady_clock;
static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[v.size() / 2]; }
static double total(const std::vector<double>& v) { double s = 0; for (double x : v) s += x; return s; }

int main(int argc, char** argv) {
    if (argc < 13) { std::printf("usage: plan_host cloud.f32 n grid_len z_len interval demand gx gy gz radius starts.f32 K\n"); return 2; }
    const size_t n = std::strtoull(argv[2], nullptr, 10);
    const float gl = std::strtof(argv[3], nullptr), zl = std::strtof(argv[4], nullptr), iv = std::strtof(argv[5], nullptr);
    const std::string demand = argv[6];
    Vector3f goal;
    for (int k = 0; k < 3; ++k) goal.d[k] = std::strtof(argv[7 + k], nullptr);
    const float radius = std::strtof(argv[10], nullptr);
    const size_t K = std::strtoull(argv[12], nullptr, 10);
    std::vector<float> cloud(3 * n), starts(3 * K);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(cloud.data(), 4, 3 * n, f) != 3 * n) { std::printf("{\"error\": \"cannot read cloud\"}\n"); return 1; }
    std::fclose(f);
    f = std::fopen(argv[11], "rb");
    if (!f || std::fread(starts.data(), 4, 3 * K, f) != 3 * K) { std::printf("{\"error\": \"cannot read starts\"}\n"); return 1; }
    std::fclose(f);
    Vector3f first;
    for (int k = 0; k < 3; ++k) first.d[k] = cloud[k];
    TwoDmap map2D(gl, zl);
    map2D.setInterval(iv);
    map2D.setCloudFirst(first);
    std::vector<double> route, exp, build, cost;
    size_t found = 0, steps = 0;
    for (size_t i = 0; i < K + 1; ++i) {               // (the first round warms up: handle creation, first-build sizing)
        const size_t q = i ? i - 1 : 0;
        Vector3f start;
        for (int k = 0; k < 3; ++k) start.d[k] = starts[3 * q + k];
        if (!map2D.create2DMap(demand, cloud.data() + 3, n - 1, 12, true)) { std::printf("{\"error\": \"%s\"}\n", map2D.lastError().c_str()); return 1; }
        RobotSphere robot(radius, start, goal);
        const auto t1 = Clock::now();
        if (!map2D.computeCost(robot.getGoal(), robot, demand)) { std::printf("{\"error\": \"%s\"}\n", map2D.lastError().c_str()); return 1; }
        const auto t2 = Clock::now();
        AstarPlanar planner(robot.getPosition(), robot.getGoal());
        const bool ok = planner.findRoute(map2D, robot, demand);
        const auto t3 = Clock::now();
        if (!i) continue;
        route.push_back(ms(t2, t3)); cost.push_back(ms(t1, t2));
        exp.push_back(map2D.timing.export_ms); build.push_back(map2D.timing.build_ms);
        found += ok ? 1 : 0; steps += planner.global_path.size();
    }
    std::printf("{\"starts\": %zu, \"found\": %zu, \"mean_route_slopes\": %.1f, \"nodes\": %llu, \"route_ms_median\": %.4f, \"route_ms_total\": %.3f, "
                "\"export_host_ms_median\": %.4f, \"route_plus_export_ms_median\": %.4f, \"build_sync_ms_median\": %.4f, "
                "\"compute_cost_and_h_copy_ms_median\": %.4f}\n",
                K, found, found ? (double)steps / (double)found : 0.0, (unsigned long long)map2D.exported().num_nodes, median(route), total(route),
                median(exp), median(route) + median(exp), median(build), median(cost));
    return 0;
}
