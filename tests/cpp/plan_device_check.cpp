// Test program for AstarPlanar::findRouteDevice of include/gndt_compat.hpp (built and run by tests/test_gpu_plan.py):
//   plan_device_check <cloud.f32> <n> <grid_len> <z_len> <interval> <demand> <gx> <gy> <gz> <sx> <sy> <sz> <radius>
// On a map built and flooded on the GPU, eager and lazy: the route findRouteDevice fills global_path with (one gndt_plan_routes call)
// is the route findRoute walks on the host afterwards, Slope object by Slope object.  findRouteDevice runs first: findRoute leaves
// g, f and fathers behind, and the device route is defined on a fresh map.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gndt_compat.hpp"

using namespace gndt_compat;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static int one_mode(bool lazy, const std::vector<float>& cloud, size_t n, float gl, float zl, float iv, const std::string& demand,
                    const Vector3f& vgoal, const Vector3f& vstart, float radius, size_t* steps) {
    const char* what = lazy ? "lazy" : "eager";
    TwoDmap M(gl, zl);
    M.setInterval(iv);
    M.setCloudFirst(Vector3f{{cloud[0], cloud[1], cloud[2]}});
    CHECK(M.create2DMap(demand, cloud.data() + 3, n - 1, 12, lazy), "%s create2DMap failed: %s", what, M.lastError().c_str());
    CHECK(M.isLazy() == lazy, "%s: wrong mode", what);
    RobotSphere robot(radius, vstart, vgoal);
    CHECK(M.computeCost(robot.getGoal(), robot, demand), "%s computeCost failed: %s", what, M.lastError().c_str());
    CHECK(M.costStats().goal_status == 0, "%s: goal status %d", what, M.costStats().goal_status);
    AstarPlanar on_device(robot.getPosition(), robot.getGoal());
    const bool found_dev = on_device.findRouteDevice(M);
    CHECK(M.lastError().empty(), "%s findRouteDevice: %s", what, M.lastError().c_str());
    AstarPlanar on_host(robot.getPosition(), robot.getGoal());
    const bool found_host = on_host.findRoute(M, robot, demand);
    CHECK(found_dev == found_host, "%s: device found %d, host found %d", what, (int)found_dev, (int)found_host);
    CHECK(on_device.global_path.size() == on_host.global_path.size(), "%s: route of %zu slopes on the device, %zu on the host", what,
          on_device.global_path.size(), on_host.global_path.size());
    auto a = on_device.global_path.begin();
    size_t k = 0;
    for (const Slope* s : on_host.global_path) {
        CHECK(*a == s, "%s: step %zu is %s/%d on the device, %s/%d on the host", what, k, (*a)->morton_xy.c_str(), (*a)->morton_z,
              s->morton_xy.c_str(), s->morton_z);
        ++a; ++k;
    }
    *steps = k;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 14) { std::printf("usage\n"); return 2; }
    const size_t n = std::strtoull(argv[2], nullptr, 10);
    const float gl = std::strtof(argv[3], nullptr), zl = std::strtof(argv[4], nullptr), iv = std::strtof(argv[5], nullptr);
    const std::string demand = argv[6];
    float goal[3], start[3];
    for (int k = 0; k < 3; ++k) { goal[k] = std::strtof(argv[7 + k], nullptr); start[k] = std::strtof(argv[10 + k], nullptr); }
    const float radius = std::strtof(argv[13], nullptr);
    std::vector<float> cloud(3 * n);
    FILE* f = std::fopen(argv[1], "rb");
    CHECK(f && std::fread(cloud.data(), 4, 3 * n, f) == 3 * n, "cannot read cloud");
    std::fclose(f);
    const Vector3f vgoal{{goal[0], goal[1], goal[2]}}, vstart{{start[0], start[1], start[2]}};
    size_t eager = 0, lazy = 0;
    if (one_mode(false, cloud, n, gl, zl, iv, demand, vgoal, vstart, radius, &eager)) return 1;
    if (one_mode(true, cloud, n, gl, zl, iv, demand, vgoal, vstart, radius, &lazy)) return 1;
    CHECK(eager == lazy && eager > 1, "eager route of %zu slopes, lazy of %zu", eager, lazy);
    std::printf("findRouteDevice == findRoute OK steps=%zu (eager and lazy)\n", eager);
    return 0;
}
