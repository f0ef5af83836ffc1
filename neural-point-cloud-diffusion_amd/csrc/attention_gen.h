// Attention kernels for head dims other than 64 (csrc/attention_gen.hip); called from the npcd_attn_* entry points of attention.hip.
#pragma once
#include "../../include/npcd_hip.h"

namespace npcd {

bool attn_gen_supported(int d);      // 32, 64, 128
// the argument block of npcd_attn_fwd / npcd_attn_bwd (16-bit dtypes only); `passes`: bit 0 = dq (+ delta), bit 1 = dk / dv
int attn_gen_fwd(const npcd_attn_args& a, void* stream);
int attn_gen_bwd(const npcd_attn_args& a, int passes, void* stream);

}  // namespace npcd
