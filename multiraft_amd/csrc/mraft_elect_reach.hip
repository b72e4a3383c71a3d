// mraft_elect_reach.hip — the election storm under a reachability mask
// (mraft_set_reachable, include/mraft.h) for gfx950: k_election_rounds_reach,
// the kernel of mraft_elect.hip with the mask's tests compiled in. Both include
// the same body (mraft_elect_kernel.inc, and through it the round body
// mraft_elect_round.inc); this one says REACH and takes the groups'
// reachability bytes, so candidate c's RequestVote reaches voter v, and v's
// reply reaches c, iff both their bits are set. The host launches it only
// while a mask is set; mraft_elect.hip holds the storm's kernels and nothing
// else.
#include "mraft_device.h"
#include "mraft_internal.h"

namespace mraft {

namespace {

template <int P>
__global__ __launch_bounds__(256) void k_election_rounds_reach(Dev s, const uint8_t *__restrict__ cand, int R,
                                                               int32_t *__restrict__ gflags,
                                                               const uint8_t *__restrict__ reach) {
  constexpr bool REACH = true;
#include "mraft_elect_kernel.inc"
}

}  // namespace

void launch_election_rounds_reach(const Dev &s, const uint8_t *cand, int R, int32_t *gflags, const uint8_t *reach,
                                  hipStream_t st) {
  const dim3 gr((unsigned)blocks_for((int64_t)s.G * 8)), bl(256);
  with_peers<1>(s.P, [&](auto pc) {
    hipLaunchKernelGGL(k_election_rounds_reach<decltype(pc)::value>, gr, bl, 0, st, s, cand, R, gflags, reach);
  });
}

}  // namespace mraft
