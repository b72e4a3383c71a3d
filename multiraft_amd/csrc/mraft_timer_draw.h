// mraft_timer_draw.h — the election timeout's stateless draw
// (include/mraft.h "timers"; RandomizedElectionTimeout, raft.go:46-50), one
// definition for the host entry point (mraft_router.cpp) and the kernels
// (mraft_clock.hip). All uint32 arithmetic.
#pragma once
#include <stdint.h>

#include "../../include/mraft.h"

#if defined(__HIPCC__)
#define MRAFT_HD __host__ __device__ __forceinline__
#else
#define MRAFT_HD inline
#endif

namespace mraft {

constexpr int32_t kTimerNowMax = 1 << 30;       // every `now` is in [0, 2^30]
constexpr int32_t kTimerElectionMax = 1 << 20;  // election_hi
constexpr int32_t kTimerHeartbeatMax = (1 << 30) - 1;

MRAFT_HD uint32_t timer_fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

MRAFT_HD bool timer_config_ok(const mraft_timer_config &c) {
  return c.heartbeat >= 1 && c.heartbeat <= kTimerHeartbeatMax && c.election_lo >= 1 &&
         c.election_lo < c.election_hi && c.election_hi <= kTimerElectionMax;
}

// election_lo + fmix(fmix(slot * 0x9E3779B9 + now) ^ seed) % (election_hi - election_lo)
MRAFT_HD int32_t timer_draw(const mraft_timer_config &c, uint32_t slot, uint32_t now) {
  const uint32_t h = timer_fmix(timer_fmix(slot * 0x9E3779B9u + now) ^ c.seed);
  return c.election_lo + (int32_t)(h % (uint32_t)(c.election_hi - c.election_lo));
}

}  // namespace mraft
