// What csrc/impala.hip takes from csrc/dqn_inplace.hip: the three kernels of the Ape-X DQN step
// that read a batch, instantiated for a replay ring read in place through the keys drawn on the
// device (conv1.h, ObsKeys; dqn_train_step_replay_rows).  launch_forward, launch_dqn_head and
// launch_backward launch them like every other learner kernel; they are compiled in a translation
// unit of their own so that impala.hip's code object stays what it is without them.
#pragma once
#include "dqn_head_step.h"
#include "lnc3.h"

namespace dqn_inplace_dev {

// conv12_fwd_s2d<T, ObsKeys> (conv1.h), T = __bf16 or float
template <typename T>
using FwdKeysKernel = void (*)(const uint8_t*, const T*, const float*, const T*, const float*, T*, uint32_t*, T*,
                               int, int, const C3Tail<T>, unsigned long long*, const ObsKeys);
// lnc3_conv12_bwd<T, ObsKeys> (lnc3.h)
template <typename T>
using BwdKeysKernel = void (*)(const float*, const T*, const float*, const float*, const T*, const T*, const T*,
                               T*, T*, float*, const uint8_t*, const T*, const T*, const uint32_t*, float*,
                               float*, int, int, const ObsKeys);
// dqn_head_step_keys_kernel<T> (dqn_head_step.h)
using HeadKeysKernel = void (*)(const DqnHeadArgs, const ObsKeys);

template <typename T> FwdKeysKernel<T> fwd_keys_kernel();
template <typename T> BwdKeysKernel<T> bwd_keys_kernel();
template <typename T> HeadKeysKernel head_keys_kernel();
template <> FwdKeysKernel<float> fwd_keys_kernel<float>();
template <> FwdKeysKernel<__bf16> fwd_keys_kernel<__bf16>();
template <> BwdKeysKernel<float> bwd_keys_kernel<float>();
template <> BwdKeysKernel<__bf16> bwd_keys_kernel<__bf16>();
template <> HeadKeysKernel head_keys_kernel<float>();
template <> HeadKeysKernel head_keys_kernel<__bf16>();

}  // namespace dqn_inplace_dev
