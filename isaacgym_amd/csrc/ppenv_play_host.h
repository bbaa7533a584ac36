// ppenv_play_host.h — ppenv_host.h plus the size bound the play accountings (ppenv_play*.hip) share.  Internal and host-only.
#pragma once
#include "../../include/ppenv_play_group.h"
#include "ppenv_host.h"

namespace {
// groups 1..PP_PLAY_GROUP_MAX, agents 1..PPENV_PLAY_MAX_AGENTS, at most 2^31 - 1 rows
inline bool pp_play_sizes_ok(int32_t envs_per_group, int32_t groups, int32_t num_agents) {
    return groups >= 1 && groups <= PP_PLAY_GROUP_MAX && envs_per_group > 0 && num_agents >= 1 && num_agents <= PPENV_PLAY_MAX_AGENTS &&
           (int64_t)envs_per_group * groups * num_agents <= INT32_MAX;
}
}  // namespace
