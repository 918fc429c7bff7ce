"""A float64 NumPy twin of rg_render, written from the spec (csrc/render.h, DESIGN.md section 4 "Render"), not from the kernel.

    frame, degenerate = render_twin(params, state, W, H, view=None, layers=None)

params: the RgScenarioParams block; state: one env's arrays -- poses [3, N], and where the scenario draws them prey_loc [P, 2],
prey_sensed [P], prey_captured [P], grid [96].  frame: uint8 [H, W, 3]; degenerate: bool [H, W], true where the pixel's centre lies
within EDGE_TOL of an edge of any drawn shape (disk rims, both edges of an outline, rectangle sides, the arena's sides, the
sides and ends of a heading segment): only there may a binary32 evaluation land on the other side.  The twin keeps its own copy
of the palette.
"""
import numpy as np

EDGE_TOL = 1e-4   # metres

LAYERS = ("arena", "zones", "markers", "rings", "robots", "heading")

PALETTE = {"background": (255, 255, 255), "surround": (224, 224, 224), "zone_a": (255, 221, 128), "zone_b": (170, 238, 153),
           "ice": (190, 230, 255), "water": (70, 130, 220), "goal": (120, 200, 120), "prey": (0, 170, 90),
           "prey_sensed": (170, 60, 200), "zone1": (230, 130, 40), "class0": (220, 40, 40), "class1": (40, 90, 220),
           "class2": (240, 190, 20), "heading": (30, 30, 30)}

PCP, WAREHOUSE, MATERIAL, SIMPLE, ARCTIC = range(5)
PREY_RADIUS = 0.025
MAX_HEADING_ANGLE = 8.0


def agent_classes(p):
    n = int(p.n_agents)
    scn = int(p.scenario)
    if scn == PCP:
        return [0 if p.sensing_radius[a] > 0 else 1 for a in range(n)]
    if scn == WAREHOUSE:
        return [a % 2 for a in range(n)]
    if scn == MATERIAL:
        n_fast = 0
        while n_fast < n and p.agent_step[n_fast] == p.agent_step[0]:
            n_fast += 1
        return [0 if a < n_fast else 1 for a in range(n)]
    if scn == ARCTIC:
        return [0 if a < 2 else 1 if a == 2 else 2 for a in range(n)]
    return [0] * n


class _Canvas(object):
    def __init__(self, wx, wy):
        self.wx, self.wy = wx, wy
        self.frame = np.empty(wx.shape + (3,), np.uint8)
        self.frame[...] = PALETTE["background"]
        self.degenerate = np.zeros(wx.shape, bool)

    def paint(self, mask, colour):
        self.frame[mask] = PALETTE[colour]

    def _box(self, u, v, u0, u1, v0, v1):
        """closed rectangle [u0, u1] x [v0, v1] in the coordinates (u, v); marks its sides"""
        t = EDGE_TOL
        near_u = (np.abs(u - u0) < t) | (np.abs(u - u1) < t)
        near_v = (np.abs(v - v0) < t) | (np.abs(v - v1) < t)
        self.degenerate |= (near_u & (v > v0 - t) & (v < v1 + t)) | (near_v & (u > u0 - t) & (u < u1 + t))
        return (u >= u0) & (u <= u1) & (v >= v0) & (v <= v1)

    def rect(self, x0, x1, y0, y1, colour):
        self.paint(self._box(self.wx, self.wy, x0, x1, y0, y1), colour)

    def outside(self, x0, x1, y0, y1, colour):
        self.paint(~self._box(self.wx, self.wy, x0, x1, y0, y1), colour)

    def disk(self, x, y, r, colour):
        if not (np.isfinite(x) and np.isfinite(y)):
            return
        d = np.hypot(self.wx - x, self.wy - y)
        self.degenerate |= np.abs(d - r) < EDGE_TOL
        self.paint(d <= r, colour)

    def outline(self, x, y, r, px, colour):
        if not (np.isfinite(x) and np.isfinite(y)):
            return
        d = np.hypot(self.wx - x, self.wy - y)
        self.degenerate |= (np.abs(d - (r + px)) < EDGE_TOL) | (np.abs(d - (r - px)) < EDGE_TOL)
        self.paint(np.abs(d - r) <= px, colour)

    def segment(self, x, y, theta, r, px, colour):
        if not (np.isfinite(x) and np.isfinite(y) and abs(theta) <= MAX_HEADING_ANGLE):
            return
        c, s = np.cos(theta), np.sin(theta)
        dx, dy = self.wx - x, self.wy - y
        self.paint(self._box(dx * c + dy * s, dy * c - dx * s, 0.0, r, -px, px), colour)


def render_twin(params, state, W, H, view=None, layers=None):
    p = params
    scn, n = int(p.scenario), int(p.n_agents)
    layers = LAYERS if layers is None else tuple(layers)
    assert all(name in LAYERS for name in layers)
    ax0, ay0, aw, ah = (float(np.float32(v)) for v in (p.bound_x0, p.bound_y0, p.bound_w, p.bound_h))
    vx0, vy0, vw, vh = (ax0, ay0, aw, ah) if view is None else (float(np.float32(v)) for v in view)
    sx, sy = vw / W, vh / H
    px = max(sx, sy)
    wx = np.broadcast_to(vx0 + (np.arange(W, dtype=np.float64) + 0.5) * sx, (H, W))
    wy = np.broadcast_to(((vy0 + vh) - (np.arange(H, dtype=np.float64) + 0.5) * sy)[:, None], (H, W))
    cv = _Canvas(wx, wy)
    poses = np.asarray(state["poses"], np.float64).reshape(3, n)
    rr = float(p.robot_diameter) / 2
    cls = agent_classes(p)

    if "arena" in layers:
        cv.outside(ax0, ax0 + aw, ay0, ay0 + ah, "surround")
    if "zones" in layers:
        if scn == WAREHOUSE:
            w = float(p.goal_width)
            cv.rect(-1.5, -1.5 + w, -1.0, 0.0, "zone_a")
            cv.rect(-1.5, -1.5 + w, 0.0, 1.0, "zone_b")
            cv.rect(1.5 - w, 1.5, -1.0, 0.0, "zone_b")
            cv.rect(1.5 - w, 1.5, 0.0, 1.0, "zone_a")
        elif scn == MATERIAL:
            w = float(p.end_goal_width)
            cv.rect(-1.5, -1.5 + w, -1.0, 1.0, "zone_a")
            cv.rect(1.5 - w, 1.5, -1.0, 1.0, "zone_b")
        elif scn == ARCTIC:
            grid = np.asarray(state["grid"]).reshape(8, 12)
            for i in range(8):
                for j in range(12):
                    if grid[i, j] > 0:
                        cv.rect(0.25 * j - 1.5, 0.25 * j - 1.25, 0.75 - 0.25 * i, 1.0 - 0.25 * i,
                                {1: "ice", 2: "water"}.get(int(grid[i, j]), "goal"))
    if "markers" in layers:
        if scn in (PCP, SIMPLE):
            loc = np.asarray(state["prey_loc"], np.float64).reshape(-1, 2)
            for j in range(int(p.num_prey)):
                if state["prey_captured"][j] == 0:
                    cv.disk(loc[j, 0], loc[j, 1], PREY_RADIUS, "prey_sensed" if state["prey_sensed"][j] != 0 else "prey")
        elif scn == MATERIAL:
            cv.outline(0.0, 0.0, float(p.zone1_radius), px, "zone1")
    if "rings" in layers and scn == PCP:
        for a in range(n):
            r = float(p.sensing_radius[a]) if p.sensing_radius[a] > 0 else float(p.capture_radius[a])
            if r > 0:
                cv.outline(poses[0, a], poses[1, a], r, px, "class%d" % cls[a])
    if "robots" in layers:
        for a in range(n):
            cv.disk(poses[0, a], poses[1, a], rr, "class%d" % cls[a])
    if "heading" in layers:
        for a in range(n):
            cv.segment(poses[0, a], poses[1, a], poses[2, a], rr, px, "heading")
    return cv.frame, cv.degenerate


def count(frame, colour):
    """pixels of `frame` [..., 3] that have the palette colour `colour`"""
    return int((np.asarray(frame) == np.asarray(PALETTE[colour], np.uint8)).all(-1).sum())
