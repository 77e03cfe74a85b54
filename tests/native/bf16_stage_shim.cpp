// catfish_amd/csrc/bf16_stage.hpp (the activation layout of the bf16 / bf16x3 kernels, decoded on the host: plain C++, no device
// work) behind a C ABI, for tests/test_bf16_stage_decode.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/bf16_stage.hpp"

extern "C" {
long long shim_stage_elems(long long n_windows, int t_len, int feats, int np) { return cf_bf16_stage_elems(n_windows, t_len, feats, np); }
int shim_frag_feature(int kb, int hh, int j) { return cf_bf16_frag_feature(kb, hh, j); }
void shim_stage_decode(const uint16_t* frag, long long n_windows, int t_len, int feats, int np, float* out) {
    cf_bf16_stage_decode(frag, n_windows, t_len, feats, np, out);
}
}
