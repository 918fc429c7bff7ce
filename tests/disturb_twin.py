"""NumPy twin of the pose disturbance (csrc/disturb.h, DESIGN.md "Pose disturbance"): the variates of a draw, the scale k of a
standard deviation, and the float32 pose update including wrap_spec.  The Philox function is tests/team_twin.py's."""
import numpy as np

from team_twin import MASK32, philox4x32_10

DISTURB_BLOCK = 0x40000000
C_MAX = 2046
C_STD = np.sqrt((2.0 ** 20 - 1.0) / 3.0)   # standard deviation of a variate: the sum of four uniforms on 0..1023


def variates(seed, ge, ep, s, a):
    """c_0 (x), c_1 (y), c_2 (theta) of the draw of (seed, global env, episode, step, agent): int32 arrays in [-2046, 2046],
    broadcast over the arguments' shapes."""
    ge, ep, s, a = np.broadcast_arrays(np.asarray(ge, np.int64), np.asarray(ep, np.int64), np.asarray(s, np.int64), np.asarray(a, np.int64))
    ge = ge.astype(np.uint64)
    blk = np.uint64(DISTURB_BLOCK) | ((s.astype(np.uint64) & np.uint64(0x3FFFFFF)) << np.uint64(4)) | a.astype(np.uint64)
    w = philox4x32_10(ge & MASK32, ge >> np.uint64(32), ep.astype(np.uint32).astype(np.uint64), blk,
                      np.uint64(seed) & MASK32, np.uint64(seed) >> np.uint64(32))
    return [sum(((wi >> np.uint32(10 * j)) & np.uint32(1023)).astype(np.int32) for wi in w) - np.int32(C_MAX) for j in range(3)]


def scale(sigma):
    """k = binary32(double(sigma) * sqrt(3.0 / 1048575.0)), sigma as the binary32 the library is handed."""
    return np.float32(np.float64(np.float32(sigma)) * np.sqrt(np.float64(3.0) / np.float64(1048575.0)))


def wrap_spec(t):
    """csrc/sim_math.h wrap_spec in float32: 2 pi (hi + lo) taken off only beyond +-pi."""
    t = np.asarray(t, np.float32)
    hi, lo, pi = np.float32(6.283185482025146484375), np.float32(-1.74845553146951715462e-07), np.float32(3.1415927410125732421875)
    dn = (t - hi) - lo
    up = (t + hi) + lo
    return np.where(t > pi, dn, np.where(t < -pi, up, t)).astype(np.float32)


def displace(poses, seed, env_offset, reset_count, episode_steps, sigma_xy, sigma_theta):
    """poses [E, 3, N] float32 displaced as the step displaces them: every operation rounded to float32, no contraction."""
    poses = np.asarray(poses, np.float32)
    E, _, N = poses.shape
    ge = (int(env_offset) + np.arange(E, dtype=np.int64))[:, None]
    ep = (np.asarray(reset_count, np.int64) - 1)[:, None]
    s = np.asarray(episode_steps, np.int64)[:, None]
    c = variates(seed, ge, ep, s, np.arange(N, dtype=np.int64)[None, :])
    kxy, kth = scale(sigma_xy), scale(sigma_theta)
    out = poses.copy()                       # k = 0 leaves that part of the pose alone: x + 0 * c would turn a -0.0 into +0.0
    if kxy != 0:
        out[:, 0] = poses[:, 0] + (kxy * c[0].astype(np.float32)).astype(np.float32)
        out[:, 1] = poses[:, 1] + (kxy * c[1].astype(np.float32)).astype(np.float32)
    if kth != 0:
        out[:, 2] = wrap_spec(poses[:, 2] + (kth * c[2].astype(np.float32)).astype(np.float32))
    return out
