// The Ape-X DQN step on a replay ring read in place (include/dqn_hip.h,
// dqn_train_step_replay_rows): the fused trunk forward, the dueling head and the fused per-frame
// backward instantiated with the device-key row map (conv1.h, ObsKeys), handed to impala.hip as
// kernel function pointers (csrc/dqn_inplace_launch.h).  A translation unit of its own, as
// ppo_replay.hip is: the code object of impala.hip -- the learner steps' kernels and where they
// sit in it -- is the same with or without them.
#include "common.h"

#include "../../include/impala_hip.h"
#include "dqn_inplace_launch.h"

namespace dqn_inplace_dev {

template <> FwdKeysKernel<float> fwd_keys_kernel<float>() { return conv12_fwd_s2d<float, ObsKeys>; }
template <> FwdKeysKernel<__bf16> fwd_keys_kernel<__bf16>() { return conv12_fwd_s2d<__bf16, ObsKeys>; }
template <> BwdKeysKernel<float> bwd_keys_kernel<float>() { return lnc3_conv12_bwd<float, ObsKeys>; }
template <> BwdKeysKernel<__bf16> bwd_keys_kernel<__bf16>() { return lnc3_conv12_bwd<__bf16, ObsKeys>; }
template <> HeadKeysKernel head_keys_kernel<float>() { return dqn_head_step_keys_kernel<float>; }
template <> HeadKeysKernel head_keys_kernel<__bf16>() { return dqn_head_step_keys_kernel<__bf16>; }

}  // namespace dqn_inplace_dev
