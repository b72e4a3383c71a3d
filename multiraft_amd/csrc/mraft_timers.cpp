// mraft_timers.cpp — the host-only part of the timers (include/mraft.h):
// the election timeout's draw as the host can compute it (to predict or check
// a deadline without a GPU, like mraft_key2shard) and the feature bitmask.
#include "../../include/mraft.h"
#include "mraft_timer_draw.h"

extern "C" {

int32_t mraft_features(void) { return MRAFT_FEATURE_TIMERS | MRAFT_FEATURE_REACH | MRAFT_FEATURE_CRASH; }

int32_t mraft_timer_draw(const mraft_timer_config *cfg, int64_t slot, int32_t now) {
  if (!cfg || !mraft::timer_config_ok(*cfg)) return -1;
  if (slot < 0 || slot > INT32_MAX || now < 0 || now > mraft::kTimerNowMax) return -1;
  return mraft::timer_draw(*cfg, (uint32_t)slot, (uint32_t)now);
}

}  // extern "C"
