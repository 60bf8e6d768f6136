// Internal launchers of the chessboard-corner detector (chessboard.hip): the reference's
// cv2.findChessboardCorners + cv2.cornerSubPix in analyze_chessboardvid (multicam_toolbox.py:22-72), as a detector of
// this project's own.  tests/chessboard_ref.py is the numpy restatement the kernels mirror.  Every launcher is
// stream-ordered (no host round trip) and returns 0, or -1 when a launch failed.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "workspace.hpp"

namespace mq {

// chess_candidates' workspace for n images of h x w; a composite stage calls the layout on its own carver
struct ChessCandBufs {
  int32_t* surv;             // survivor map (n, h, w)
  uint32_t* hist;            // (n, 256)
  void* st;                  // select state (n), chessboard.hip's SelState
  unsigned long long* keys;  // (n, next power of two >= K)
};
ChessCandBufs chess_candidates_layout(Carver& c, int n, int h, int w, int K);
size_t chess_candidates_ws_bytes(int n, int h, int w, int K);

// gray uint8 (n, h, w) -> resp int32 (n, h, w): ChESS on the 3 x 3 binomial blur, 0 in the 5-pixel border
int chess_response(const uint8_t* gray, int n, int h, int w, int32_t* resp, hipStream_t s);

// resp -> pos int32 (n, K, 2) [x, y], val int32 (n, K), count int32 (n): the 9 x 9 maxima with R > 0, the first K
// under (R descending, y ascending, x ascending); rows past count are zero.  1 <= K <= 1024; h * w < 2^31.
int chess_candidates(const int32_t* resp, int n, int h, int w, int K, int32_t* pos, int32_t* val, int32_t* count,
                     const ChessCandBufs& b, hipStream_t s);

// candidates -> found int32 (n), corners float64 (n, 54, 2) in full-frame pixels (NaN when not found), idx int32
// (n, 54) candidate indices (-1 when not found; may be null)
int chess_grid(const int32_t* pos, const int32_t* val, const int32_t* count, int n, int K, double scale,
               int32_t* found, double* corners, int32_t* idx, hipStream_t s);

// cornerSubPix on corners float64 (n, per_img, 2), in place, image i of gray uint8 (n, h, w); found (n) or null:
// the corners of an image with found[i] == 0 are set to NaN.  1 <= win <= 16.
int corner_subpix(const uint8_t* gray, int n, int h, int w, double* corners, int per_img, const int32_t* found,
                  int win, int max_iter, double eps, hipStream_t s);

}  // namespace mq
