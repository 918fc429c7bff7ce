"""float64 twin of the lidar observation (marbler_amd/csrc/lidar.h; DESIGN.md "Lidar"), for tests/test_lidar_config.py and
tests/test_gpu_lidar.py.  Straight from the spec: per ray, every candidate distance (two walls, every other robot's disk)
computed in binary64 from the binary32 poses, the smallest positive one taken.  Also says which rays are degenerate -- a
binary32 evaluation may legitimately land on the other side of a decision there: a grazing discriminant, two candidates within
EPS of each other, a range within EPS of L, a centre within EPS of a disk's rim or of the arena's edge (GRAZE, EPS below)."""
import numpy as np

EPS = 1e-5
# a grazing ray: |b^2 - cc| below GRAZE m^2.  The kernel forms the discriminant as rho^2 - p^2 (p the partner's distance across
# the ray: error ~1e-8 m^2), so its range is off by ~1e-8 / (2 sqrt(disc)): at GRAZE, 5e-6 -- inside the tests' 2e-5
GRAZE = 1e-6


def directions(R):
    a = 2.0 * np.pi * np.arange(R, dtype=np.float64) / R
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32).astype(np.float64)


def lidar_env(x, y, th, R, L, rho, bounds, eps=EPS):
    """One env: x, y, th [N] (the stored binary32 poses).  bounds = (x0, x1, y0, y1).  Returns (values [N, R] float64 =
    min(t, L) / L, degenerate [N, R] bool)."""
    x, y, th = (np.asarray(v, dtype=np.float64) for v in (x, y, th))
    x0, x1, y0, y1 = (float(b) for b in bounds)
    N = len(x)
    d = directions(R)
    val = np.zeros((N, R))
    deg = np.zeros((N, R), dtype=bool)
    for i in range(N):
        out_d = min(x[i] - x0, x1 - x[i], y[i] - y0, y1 - y[i])
        if out_d < 0.0:
            deg[i] = out_d > -eps
            continue   # every ray 0
        c, s = np.cos(th[i]), np.sin(th[i])
        others = [j for j in range(N) if j != i]
        dx, dy = x[others] - x[i], y[others] - y[i]
        cc = dx * dx + dy * dy - rho * rho
        if np.any(cc <= 0.0):
            deg[i] = np.any(np.abs(cc) < eps)
            continue   # inside a partner's disk: every ray 0
        near_rim = np.any(np.abs(cc) < eps)
        for k in range(R):
            ux = c * d[k, 0] - s * d[k, 1]
            uy = s * d[k, 0] + c * d[k, 1]
            cand = []
            if ux > 0:
                cand.append((x1 - x[i]) / ux)
            elif ux < 0:
                cand.append((x0 - x[i]) / ux)
            if uy > 0:
                cand.append((y1 - y[i]) / uy)
            elif uy < 0:
                cand.append((y0 - y[i]) / uy)
            grazing = False
            for m in range(len(others)):
                b = dx[m] * ux + dy[m] * uy
                disc = b * b - cc[m]
                if abs(disc) < GRAZE and b > 0:
                    grazing = True
                if disc >= 0.0 and b > 0.0:
                    cand.append(b - np.sqrt(disc))
            cand = sorted(cand)
            t = cand[0]
            val[i, k] = min(t, L) / L
            close = len(cand) > 1 and cand[1] - cand[0] < eps and cand[0] < L + eps
            deg[i, k] = grazing or close or abs(t - L) < eps or near_rim
    return val, deg


def lidar_batch(poses, R, L, rho, bounds, eps=EPS):
    """poses [E, 3, N] (x row, y row, theta row: rg_state.poses) -> (values [E, N, R], degenerate [E, N, R])."""
    poses = np.asarray(poses)
    E = poses.shape[0]
    vals, degs = [], []
    for e in range(E):
        v, g = lidar_env(poses[e, 0], poses[e, 1], poses[e, 2], R, L, rho, bounds, eps)
        vals.append(v)
        degs.append(g)
    return np.stack(vals), np.stack(degs)


def bounds_of(params):
    x0, y0 = np.float32(params.bound_x0), np.float32(params.bound_y0)
    return (float(x0), float(np.float32(x0 + np.float32(params.bound_w))), float(y0), float(np.float32(y0 + np.float32(params.bound_h))))
