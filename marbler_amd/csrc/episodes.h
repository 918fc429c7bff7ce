// episodes.h -- the rule of rg_episodes_append (include/robogym.h), stated once: how a collector's time-major stream becomes
// episode-major slots padded to episode_limit + 1 (the layout of EPyMARL's EpisodeBatch / ReplayBuffer).  DESIGN.md section 4
// "Episode buffer" is the same rule in prose; tests/episodes_twin.py is it in NumPy.
//
// Shapes.  A buffer has E envs, R >= 1 slots per env, episode limit L >= 1, N agents, row width D; slot s = e R + r.  All of it
// caller-owned device memory (rg_episode_buffer):
//     obs [E R][L + 1][N][D] f32      actions [E R][L + 1][N] i32      reward [E R][L + 1] f32
//     terminated, filled [E R][L + 1] u8                               prob [E R][L + 1][N] f32 (optional)
//   per slot   length i32, episode_return f32, complete u8, fresh u8, episode_index i32 (which of env e's episodes it holds)
//   per env    cursor [E][4] i32: the open slot (s, or -1 for none), the position in it, the number of episodes opened (and
//              not abandoned), the overflow counter.
// The stream is what BatchedRunner.run(T) returns (rg_episode_stream): obs [T + 1][E][N][D], actions [T][E][N], reward [T][E],
// terminated [T][E] u8, episode_start [T][E] u8, optional prob [T][E][N].
//
// Semantics.  For every env e independently, for t = 0 .. T - 1 in order:
//   1 If episode_start[t, e]: an episode that is still open is ABANDONED -- its slot is not marked complete, it does not count
//     as opened, and the new episode takes its place (the same slot, the same episode_index).  The new episode opens in slot
//     e R + (opened mod R) at position 0, and `opened` goes up.  Opening zeroes the slot's filled, terminated and reward rows
//     (all L + 1), its length, episode_return, complete and fresh, and sets episode_index.  obs / actions / prob rows keep what
//     they held: `filled` says which rows are data.
//   2 If the env has no open episode the transition is dropped (a buffer attached in the middle of an episode discards the
//     part it sees of it).
//   3 Otherwise, at position p: row p of the slot takes obs[t, e], actions[t, e], reward[t, e], terminated[t, e] (as 0 / 1) and
//     prob[t, e]; filled[p] = 1; episode_return = episode_return + reward[t, e], ONE binary32 addition per step, in step order.
//   4 If terminated[t, e]: row p + 1 takes obs[t + 1, e] and filled[p + 1] = 1 (EPyMARL's last-data slot; with the runner's
//     zero_obs_on_end it is the reset observation, which the learners mask out).  length = p + 1, complete = fresh = 1, the
//     episode closes (cursor: no open slot).
//   5 Else if p + 1 == L (a stream with a longer horizon than the buffer): the episode is force-closed exactly as in 4 --
//     terminated[p] stays 0 -- and the env's overflow counter goes up.  Else the position becomes p + 1.
// Nothing is ever written outside a slot: a position never reaches L, so the last row written is L.
//
// Ring wrap-around.  An env that opens more than R episodes in one call overwrites its own older slots; the result is that of
// the sequential rule.  The kernel keeps it by construction: ONE wave owns an env for the whole call and walks its episodes in
// order (robogym_episodes.hip), so two episodes that share a slot are never written side by side.
#pragma once
#include <stdint.h>

#include "../../include/robogym.h"

namespace rg {
namespace episodes {

constexpr int BLOCK = 256;              // lanes of a work-group: four waves, an env each
constexpr int ENVS_PER_BLOCK = BLOCK / 64;
constexpr int COPY_UNROLL = 4;          // row pieces a lane has in flight in the row copy
// cursor [E][4]
enum { CUR_OPEN = 0, CUR_POS = 1, CUR_OPENED = 2, CUR_OVERFLOW = 3, CUR_WORDS = 4 };

struct Args {
    rg_episode_buffer b;
    rg_episode_stream s;
};

}  // namespace episodes
}  // namespace rg
