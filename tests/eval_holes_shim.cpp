// Host build of the novel-view hole rule of splatam_amd/csrc/eval_math.h for tests/test_novel_view_cpu.py: the very functions the
// metric kernel calls per pixel (eval_hole) and the validity rule a caller applies to the count (eval_nvs_valid).
#include "../splatam_amd/csrc/splat_math.h"
#include "../splatam_amd/csrc/eval_math.h"

using namespace splat;

extern "C" {

// number of holes among n pixels; flags[i] = 1 where pixel i is one
long long eh_count(int n, const float *gt_depth, const float *sil, float sil_thres, unsigned char *flags) {
    long long holes = 0;
    for (int i = 0; i < n; ++i) {
        const bool h = eval_hole(gt_depth[i], sil[i], sil_thres);
        flags[i] = h ? 1 : 0;
        holes += h ? 1 : 0;
    }
    return holes;
}

int eh_valid(long long holes, int W, int H) { return eval_nvs_valid(holes, W, H) ? 1 : 0; }

int eh_sum_slot(void) { return kEvalSumHoles; }

}  // extern "C"
