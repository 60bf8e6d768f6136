// Internal interface of the baseline JPEG decoder (jpeg_dec.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "jpeg_dec_dev.hpp"

namespace mq {

// What depends on the header only: built on the host, passed to the kernels by value.
struct JpegDecGeom {
  int H, W, n_comp;
  int h, v;                 // luma sampling (1 x 1 for one component)
  int n_luma, n_blocks;     // blocks per MCU
  int mcus_x, mcus_y, n_mcu;
  int ri, n_int;            // MCUs per interval (n_mcu when the stream has no restart markers), intervals
  int y_stride, c_stride;   // bytes per row of the MCU-padded planes
  int64_t y_bytes, c_bytes; // bytes per frame of a plane
  int cw, ch;               // the true chroma extent ceil(W / h) x ceil(H / v)
  int fancy;                // h == 2 and cw > 2: libjpeg's interpolating upsampler, else replication
};

// 0, or -2 for an info that mq_jpeg_parse could not have filled
int jpeg_dec_geom(const mq_jpeg_info& info, JpegDecGeom& g);
size_t jpeg_dec_workspace_bytes(int n, const JpegDecGeom& g);
// the memset and the four kernels on stream s; -5 if the ws_bytes at ws are fewer than jpeg_dec_workspace_bytes
int jpeg_decode(const uint8_t* streams, int64_t stream_stride, const int32_t* sizes, int n, const mq_jpeg_info& info,
                const JpegDecGeom& g, uint8_t* frames, int64_t frame_stride, int32_t* status, void* ws, size_t ws_bytes,
                hipStream_t s);

}  // namespace mq
