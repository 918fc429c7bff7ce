"""NumPy twin of the team pool's index draw (csrc/team.h team_draw): Philox4x32-10 at block 0x80000000 of the reset sampler's
stream family, t = (uint64(w0) * C) >> 32 in the episode mode, env_offset + e mod C in the fixed mode."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
TEAM_BLOCK = 0x80000000
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over arrays of counters (uint32 words); returns the four output words."""
    c = [np.asarray(v, np.uint64) & MASK32 for v in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, np.uint64) & MASK32
    k1 = np.asarray(k1, np.uint64) & MASK32
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK32, p1 & MASK32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK32, p0 & MASK32]
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return [v.astype(np.uint32) for v in c]


def team_index(seed, ge, episode, n_sets, mode=0):
    """Team index of the episode `episode` (the reset_count value the reset sampler draws it with) of global env `ge`."""
    ge = np.asarray(ge, np.uint64)
    if mode == 1:
        return (ge % np.uint64(n_sets)).astype(np.int32)
    ep = np.asarray(episode, np.int64).astype(np.uint32).astype(np.uint64)
    w = philox4x32_10(ge & MASK32, ge >> np.uint64(32), ep, np.full(ge.shape, TEAM_BLOCK, np.uint64),
                      np.uint64(seed) & MASK32, np.uint64(seed) >> np.uint64(32))
    return ((w[0].astype(np.uint64) * np.uint64(n_sets)) >> np.uint64(32)).astype(np.int32)


def expected_after_reset(seed, env_offset, reset_count, n_sets, mode=0):
    """Every env's index after its latest episode start: the episode it runs is reset_count - 1."""
    rc = np.asarray(reset_count, np.int64)
    return team_index(seed, env_offset + np.arange(len(rc)), rc - 1, n_sets, mode)
