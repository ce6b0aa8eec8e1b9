// Host build of splatam_amd/csrc/lpips_math.h for tests/test_lpips_cpu.py: the header's functions behind C names, nothing else.
#include "../splatam_amd/csrc/lpips_math.h"

using namespace splat;

extern "C" {

int lm_layers(void) { return kLpipsLayers; }
int lm_min_size(void) { return kLpipsMinSize; }
// layer l: cin, cout, k, stride, pad, pool
void lm_layer(int l, int *out) {
    const LpipsLayer L = lpips_layer(l);
    out[0] = L.cin; out[1] = L.cout; out[2] = L.k; out[3] = L.stride; out[4] = L.pad; out[5] = L.pool;
}
int lm_conv_out(int n, int k, int stride, int pad) { return lpips_conv_out(n, k, stride, pad); }
int lm_pool_out(int n) { return lpips_pool_out(n); }
int lm_layer_in(int n, int l) { return lpips_layer_in(n, l); }
int lm_tap_size(int n, int l) { return lpips_tap_size(n, l); }
int lm_tap_rows(int W, int H, int l) { return lpips_tap_rows(W, H, l); }
int lm_layer_K(int l) { return lpips_layer_K(l); }
int lm_layer_Kpad(int l) { return lpips_layer_Kpad(l); }
// the k order of the implicit GEMM for a KH x KH window: out = (c, dy, dx); returns 0 for a window size no layer has
int lm_k_map(int kh, int k, int *out) {
    if (kh == 11) lpips_k_map<11>(k, out, out + 1, out + 2);
    else if (kh == 5) lpips_k_map<5>(k, out, out + 1, out + 2);
    else if (kh == 3) lpips_k_map<3>(k, out, out + 1, out + 2);
    else return 0;
    return 1;
}
long long lm_weight_offset(int l) { return (long long)lpips_weight_offset(l); }
long long lm_bias_offset(int l) { return (long long)lpips_bias_offset(l); }
long long lm_lin_offset(int l) { return (long long)lpips_lin_offset(l); }
long long lm_weight_floats(void) { return (long long)lpips_weight_floats(); }
long long lm_pack_offset(int l) { return (long long)lpips_pack_offset(l); }
long long lm_pack_bias_offset(int l) { return (long long)lpips_pack_bias_offset(l); }
long long lm_pack_lin_offset(int l) { return (long long)lpips_pack_lin_offset(l); }
long long lm_pack_floats(void) { return (long long)lpips_pack_floats(); }
float lm_input(float v, int ch) { return lpips_input(v, ch); }
float lm_input_masked(float v, int ch, float gt_depth, float sil, float sil_thres, int sil_mask) {
    return lpips_input_masked(v, ch, gt_depth, sil, sil_thres, sil_mask != 0);
}

}  // extern "C"
