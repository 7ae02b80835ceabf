// evalmatch.hip — the matching step of the VOC evaluation (eval.py:278-292 with filter_valid, filter_cls_data, filter_cls_pred, matching,
// _matching) for a whole batch in ONE launch: y2_eval_match (include/yolo2_hip.h).
//
// This is a latency kernel, not a throughput kernel: per image it evaluates at most M x G IoUs (3.2e4 for M = 200 x 20 expanded detections against G = 8 labels),
// which is nothing.  What it removes is the reference's shape of the work: one IoU launch, two blocking device-to-host copies and a Python claim
// loop per (image, predicted class) - several hundred round trips for a batch of 32 VOC images - become one launch without a synchronisation.
// Compiled with -ffp-contract=off like detect.hip: the IoU is common.h's iou_one, the same device function y2_iou_rowmax runs.
#include "common.h"

namespace {

struct EvalMatchArgs {
    const float* det_min; const float* det_max; const long long* det_cls; const int32_t* det_count;      // [B][M][2] x 2, [B][M], [B]
    const float* gt_min; const float* gt_max; const long long* gt_cls; const uint8_t* gt_difficult;     // [B][G][2] x 2, [B][G], [B][G]
    uint8_t* tp; int32_t* cls_num;                                                                       // [B][M], [C]
    int M, G, C;
    float thr, min_union;
};

constexpr int EM_FREE = 0x7fffffff;      // claim slot of a ground-truth box no positive row points at

// One workgroup per image.  LDS (32 bytes per ground-truth box): box [G][4], class [G] (int64 like the labels), valid [G], claim [G].
// Pass 1 (rows strided over the 256 threads): tp[i] = 0; a participating row finds its best valid same-class box (first maximum, array order) and,
// when positive, lowers claim[argmax] to its row index with an LDS atomicMin - claim[g] ends as the EARLIEST positive row whose arg-max is g, in
// whatever order the threads arrive: integer minimum, bit-reproducible.
// Pass 2 (after the barrier): row i is a true positive iff it is positive and claim[argmax(i)] == i, i.e. iff some claim slot holds i - so the
// slots are scattered (tp[claim[g]] = 1) instead of keeping or recomputing (positive, argmax) per row, whose number M is unbounded.
__global__ __launch_bounds__(256) void eval_match_kernel(const EvalMatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char em_smem[];
    const int G = a.G, M = a.M;
    long long* g_cls = reinterpret_cast<long long*>(em_smem);                 // [G]
    float* g_box = reinterpret_cast<float*>(g_cls + G);                        // [G][4] ymin xmin ymax xmax
    int* g_valid = reinterpret_cast<int*>(g_box + 4 * (size_t)G);              // [G]
    int* g_claim = g_valid + G;                                                // [G]
    const int b = blockIdx.x, t = threadIdx.x;
    for (int g = t; g < G; g += 256) {
        const size_t o = (size_t)b * G + g;
        const float y0 = a.gt_min[2 * o], x0 = a.gt_min[2 * o + 1], y1 = a.gt_max[2 * o], x1 = a.gt_max[2 * o + 1];
        const long long c = a.gt_cls[o];
        const bool valid = y0 < y1 && x0 < x1 && a.gt_difficult[o] < 1;       // eval.py:141 (zero padding is invalid by itself)
        g_box[4 * g] = y0; g_box[4 * g + 1] = x0; g_box[4 * g + 2] = y1; g_box[4 * g + 3] = x1;
        g_cls[g] = c;
        g_valid[g] = valid ? 1 : 0;
        g_claim[g] = EM_FREE;
        if (valid && c >= 0 && c < a.C) atomicAdd(&a.cls_num[c], 1);          // eval.py:280-281
    }
    __syncthreads();
    int count = a.det_count[b];
    count = count < 0 ? 0 : (count > M ? M : count);
    uint8_t* tp = a.tp + (size_t)b * M;
    for (int i = t; i < M; i += 256) {
        tp[i] = 0;
        if (i >= count) continue;
        const size_t o = (size_t)b * M + i;
        const float y0 = a.det_min[2 * o], x0 = a.det_min[2 * o + 1], y1 = a.det_max[2 * o], x1 = a.det_max[2 * o + 1];
        const long long c = a.det_cls[o];
        float bv = 0.f;
        int bi = -1;
        for (int g = 0; g < G; ++g) {
            if (!g_valid[g] || g_cls[g] != c) continue;
            const float v = iou_one(y0, x0, y1, x1, g_box[4 * g], g_box[4 * g + 1], g_box[4 * g + 2], g_box[4 * g + 3], a.min_union);
            if (bi < 0 || v > bv) { bv = v; bi = g; }                          // first maximum, like iou_rowmax_kernel over the class's boxes
        }
        if (bi >= 0 && bv > a.thr) atomicMin(&g_claim[bi], i);                 // eval.py:71 (strict, fp32) and :57-64
    }
    __syncthreads();
    for (int g = t; g < G; g += 256) {
        const int i = g_claim[g];
        if (i != EM_FREE) tp[i] = 1;                                            // distinct slots hold distinct rows: one writer per byte
    }
}

}  // namespace

extern "C" int y2_eval_match(const float* det_min, const float* det_max, const long long* det_cls, const int32_t* det_count,
                             const float* gt_min, const float* gt_max, const long long* gt_cls, const uint8_t* gt_difficult,
                             int B, int M, int G, int C, float threshold, float min_union, uint8_t* tp, int32_t* cls_num, y2_stream_t stream) {
    if (B <= 0 || M < 0 || G < 0 || C <= 0 || !det_count || !cls_num) return Y2_EINVAL;
    if (M > 0 && (!det_min || !det_max || !det_cls || !tp)) return Y2_EINVAL;
    if (G > 0 && (!gt_min || !gt_max || !gt_cls || !gt_difficult)) return Y2_EINVAL;
    if (G > Y2_EVAL_MATCH_MAX_G) return Y2_ENOSUP;
    EvalMatchArgs a;
    a.det_min = det_min; a.det_max = det_max; a.det_cls = det_cls; a.det_count = det_count;
    a.gt_min = gt_min; a.gt_max = gt_max; a.gt_cls = gt_cls; a.gt_difficult = gt_difficult;
    a.tp = tp; a.cls_num = cls_num; a.M = M; a.G = G; a.C = C; a.thr = threshold; a.min_union = min_union;
    Y2_LAUNCH("eval_match_kernel", 0.0, eval_match_kernel, dim3(B), dim3(256), (size_t)G * 32, y2_s(stream), a);
    Y2_LAUNCH_CHECK();
    return Y2_OK;
}
