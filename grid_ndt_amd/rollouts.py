"""Candidate trajectories for TwoDmap.walk_paths and the choice among the walked ones: the two ends of a local planner's loop.

    seg = m.segment_scan(frame, max_clusters=64)             # what in this frame is not in the map: a pallet, a person, a cart
    field = m.obstacle_field(seg, base=clearance)            # hops to them for every slope, minimised with the map's own barriers
    paths = rollouts.arcs(pose, v, omegas, dt, T)            # a DWA fan from the robot's pose
    info = m.walk_paths(paths, hops=field, min_hops=2)       # driven over the map on the device, stopped where a path comes too close
    best = rollouts.choose(info, h[info["end_row"]])         # h: the cost map of the last computeCost, per row
    stance = m.footprints_along(paths[info["status"] == 0], 0.3, 0.2)   # for a vehicle: the footprint along the arcs that survive

Plain tensor arithmetic: nothing here is a hot path."""
import numpy as np


def arcs(pose_xyz_yaw, v, omegas, dt, T):
    """Unicycle arcs from one pose: [K, T, 3] float32 on the pose's device (a torch tensor in, a torch tensor out; anything else numpy).
    pose_xyz_yaw = (x, y, z, yaw); the K arcs drive at speed v with the turn rates `omegas` (rad/s), waypoint j at time j * dt, waypoint 0
    the pose itself.  Closed form: x + v/w (sin(yaw + w t) - sin yaw), y - v/w (cos(yaw + w t) - cos yaw); the straight line where
    |w| < 1e-6.  z is the pose's for every waypoint (a walk only reads waypoint 0's)."""
    torch_in = hasattr(pose_xyz_yaw, "device") and hasattr(pose_xyz_yaw, "dtype") and not isinstance(pose_xyz_yaw, np.ndarray)
    if torch_in:
        import torch as xp
        pose = pose_xyz_yaw.to(xp.float64)
        w = xp.as_tensor(omegas, dtype=xp.float64, device=pose.device).reshape(-1, 1)
        t = xp.arange(int(T), dtype=xp.float64, device=pose.device).reshape(1, -1) * float(dt)
    else:
        xp = np
        pose = np.asarray(pose_xyz_yaw, np.float64)
        w = np.asarray(omegas, np.float64).reshape(-1, 1)
        t = np.arange(int(T), dtype=np.float64).reshape(1, -1) * float(dt)
    x0, y0, z0, yaw = pose[0], pose[1], pose[2], pose[3]
    straight = xp.abs(w) < 1e-6
    ws = xp.where(straight, xp.ones_like(w), w)
    th = yaw + w * t
    x = xp.where(straight, x0 + v * t * xp.cos(yaw), x0 + (v / ws) * (xp.sin(th) - xp.sin(yaw)))
    y = xp.where(straight, y0 + v * t * xp.sin(yaw), y0 - (v / ws) * (xp.cos(th) - xp.cos(yaw)))
    z = xp.zeros_like(x) + z0
    out = xp.stack([x, y, z], -1)
    return out.float() if torch_in else out.astype(np.float32)


def choose(info, h_end):
    """The index of the path to drive: among the paths of walk_paths' `info` whose status is done (0), the one with the least h_end —
    the cost map's h at the path's end_row, [K] — ties broken by the shorter `length`, then the lower index; -1 if no path is done."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    status, length, h = to_np(info["status"]), to_np(info["length"]).astype(np.float64), to_np(h_end).astype(np.float64)
    done = np.flatnonzero(status == 0)
    if done.size == 0:
        return -1
    order = np.lexsort((done, length[done], h[done]))
    return int(done[order[0]])


def headings(paths):
    """Footprint poses along K paths of T waypoints ([K, T, 3] or [K, T, 4], walk_paths' layout): [K, T, 5] float32 x, y, z, hx, hy
    for TwoDmap.footprints (torch in, torch out on the same device; anything else numpy).  A path ends at its first waypoint whose x
    or y is not finite; (hx, hy) is the vector to the next waypoint of the path, in fp32, the last waypoint repeats its predecessor's
    heading (a path of one waypoint looks along +x), and the waypoints at and behind the end are NaN: bad poses, which
    footprints_along leaves out of its verdict.  Two waypoints in one place give the zero vector, a bad pose that does count."""
    torch_in = hasattr(paths, "device") and hasattr(paths, "dtype") and not isinstance(paths, np.ndarray)
    if torch_in:
        import torch as xp
        p = paths[..., :3].float()
        K, T = int(p.shape[0]), int(p.shape[1])
        col = lambda v: xp.full((K, 1, 2), v, dtype=xp.float32, device=p.device)
        live = xp.cumprod((xp.isfinite(p[..., 0]) & xp.isfinite(p[..., 1])).to(xp.int32), 1).bool()
        off = xp.zeros((K, 1), dtype=xp.bool, device=p.device)
        cat = xp.cat
    else:
        xp = np
        p = np.asarray(paths, np.float32)[..., :3]
        K, T = p.shape[0], p.shape[1]
        col = lambda v: np.full((K, 1, 2), v, np.float32)
        live = np.cumprod(np.isfinite(p[..., 0]) & np.isfinite(p[..., 1]), 1).astype(bool)
        off = np.zeros((K, 1), bool)
        cat = np.concatenate
    if T == 0:
        return cat([p, p[..., :2]], -1)
    has_next = cat([live[:, 1:], off], 1)
    step = cat([p[:, 1:, :2] - p[:, :-1, :2], col(0.0)], 1)
    h = xp.where(has_next[..., None], step, xp.zeros_like(step))
    ahead = col(0.0)
    ahead[:, :, 0] = 1.0
    prev = cat([ahead, h[:, :-1]], 1)
    h = xp.where((live & ~has_next)[..., None], prev, h)
    out = cat([p, h], -1)
    return xp.where(live[..., None], out, xp.full_like(out, float("nan")))


def view_directions(h_fov, v_fov, n_h, n_v):
    """Unit vectors of a sensor's fan for TwoDmap.view_gain / cast_scan: float32 [n_h * n_v, 3] in the sensor frame (x forward, y left,
    z up), direction iv * n_h + ih = (cos e cos a, cos e sin a, sin e) with the azimuths a spread evenly over the horizontal field of
    view h_fov and the elevations e over the vertical one v_fov (radians, both centred on the x axis; n = 1 looks along it).  A
    full turn (h_fov >= 2 pi) leaves out its far end, which is its near end again."""
    def spread(fov, n):
        n = int(n)
        if n <= 1:
            return np.zeros(max(n, 0))
        if fov >= 2.0 * np.pi:
            return -np.pi + np.arange(n) * (2.0 * np.pi / n)
        return np.linspace(-0.5 * fov, 0.5 * fov, n)
    a, e = spread(float(h_fov), n_h), spread(float(v_fov), n_v)
    ce = np.cos(e)[:, None]
    d = np.stack([ce * np.cos(a)[None, :], ce * np.sin(a)[None, :], np.broadcast_to(np.sin(e)[:, None], (len(e), len(a)))], 2)
    return np.ascontiguousarray(d.reshape(-1, 3), np.float32)
