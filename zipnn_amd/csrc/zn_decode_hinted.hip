// zn_decode_hinted.hip — the hinted instances of the fused decoder: zn_k_decode_hinted<P, 1> reads, <P, 2> writes the sidecar index of sub-block
// start positions that a resident store keeps beside a body; zn_k_hint_size sizes it.  The kernels are the templates of zn_decode_fused.hip, instantiated in a
// translation unit of their own so that they compile beside the existing instances (and cannot disturb them): that file, with its host side switched off.
#define ZN_DECODE_HINTED_TU 1
#include "zn_decode_fused.hip"
