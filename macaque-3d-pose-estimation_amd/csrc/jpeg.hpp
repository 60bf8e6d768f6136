// Internal interface of the baseline JPEG encoder (jpeg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mq {

constexpr int JPEG_HEADER_BYTES = 629;          // SOI .. SOS, the same for every (H, W, quality, RI)
constexpr int JPEG_BLOCK_MAX_BITS = 20 + 63 * 26;  // DC 9 + 11 bits, 63 AC of 16 + 10 bits
constexpr int JPEG_MAX_RI = 32;

// What depends on (H, W, quality, RI) only: built on the host, passed to the kernels by value.
struct JpegHeader {
  uint8_t bytes[JPEG_HEADER_BYTES + 3];
};
struct JpegQuant {
  uint32_t recip[2][64];  // ceil(2^20 / Q), natural order; [0] luma, [1] chroma
  uint8_t q[2][64];       // Q
};

// bytes of one restart interval's slot in the scratch buffer: its worst-case bits, every byte stuffed
inline size_t jpeg_slot_bytes(int ri) { return 2 * (((size_t)ri * 6 * JPEG_BLOCK_MAX_BITS + 7) / 8); }
inline int64_t jpeg_n_mcu(int H, int W) { return (int64_t)((H + 15) / 16) * ((W + 15) / 16); }
inline int64_t jpeg_n_intervals(int H, int W, int ri) { return (jpeg_n_mcu(H, W) + ri - 1) / ri; }
size_t jpeg_max_bytes(int H, int W, int ri);
size_t jpeg_workspace_bytes(int n, int H, int W, int ri);
// 0, or -2 on a quality outside [1, 100]
int jpeg_make_header(int H, int W, int quality, int ri, JpegHeader& hdr, JpegQuant& q);
// the three stages on stream s; -5 if the ws_bytes at ws are fewer than jpeg_workspace_bytes
int jpeg_encode(const uint8_t* frames, int64_t frame_stride, int n, int H, int W, int ri, const JpegHeader& hdr,
                const JpegQuant& q, uint8_t* out, int64_t out_stride, int32_t* out_size, void* ws, size_t ws_bytes,
                hipStream_t s);

}  // namespace mq
