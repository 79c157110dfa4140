// Box arithmetic shared by the kernels that move boxes from the letterboxed batch to the original image (ly_val_match in ly_metrics.hip,
// ly_scale_boxes in ly_letterbox.hip).  Both files are compiled with -ffp-contract=off: the subtraction and the division are the float32
// operations the reference performs, in its order.
#pragma once
#include <hip/hip_runtime.h>

// scale_boxes + clip_boxes (utils/general.py:800-829): (x - pad) / gain, clamped to the native image
__device__ __forceinline__ float ly_val_native(float v, float pad, float gain, float hi) {
  v = (v - pad) / gain;
  return v < 0.f ? 0.f : (v > hi ? hi : v);
}
