// Internal launcher of the bilinear resize kernel (resize.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq {

// uint8 BGR (n, H, W, 3) -> (n, h, w, 3); strides in bytes between images, rows packed
int resize_bilinear(const uint8_t* src, int64_t src_stride, int n, int H, int W, uint8_t* dst, int64_t dst_stride, int h,
                    int w, hipStream_t s);

}  // namespace mq
