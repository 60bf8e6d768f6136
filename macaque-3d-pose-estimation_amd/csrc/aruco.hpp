// Internal launchers of the ArUco-marker detector (aruco.hip): the reference's aruco.detectMarkers in
// analyze_aruco_marker_vid / analyze_aruco_cube_vid (multicam_toolbox.py:244-391), as a detector of this project's
// own.  tests/aruco_ref.py is the numpy restatement the kernels mirror.  Every launcher is stream-ordered (no host
// round trip) and returns 0, or -1 when a launch failed.  h * w < 2^31.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "workspace.hpp"

namespace mq {

// gray uint8 (n, h, w) -> dark uint8 (n, h, w): 1 where gray * 529 < boxsum - 7 * 529 over the 23 x 23 window
int aruco_threshold(const uint8_t* gray, int n, int h, int w, uint8_t* dark, hipStream_t s);

// dark -> labels int32 (n, h, w): the smallest linear index of the pixel's 4-connected component, -1 where light
int aruco_label(const uint8_t* dark, int n, int h, int w, int32_t* labels, hipStream_t s);

// aruco_components' workspace for n images of h x w; a composite stage calls the layout on its own carver
struct ArucoCompBufs {
  int32_t* area;     // (n, h, w) pixel count at each component's label
  void* slots;       // (n, max slots of h x w), aruco.hip's Slot
  size_t n_area;
  int32_t* n_slots;  // (n)
};
ArucoCompBufs aruco_components_layout(Carver& c, int n, int h, int w);
size_t aruco_components_ws_bytes(int n, int h, int w);

// labels -> count int32 (n): the components that pass the gates; cand int32 (n, max_quads, 16): the first max_quads
// of them in ascending label order (label, area, x0, y0, x1, y1, 8 extreme pixels), rows past the count zero
int aruco_components(const int32_t* labels, int n, int h, int w, int max_quads, int32_t* count, int32_t* cand,
                     const ArucoCompBufs& b, hipStream_t s);

// candidates -> ok / ids / rot int32 (n, max_quads), corners float64 (n, max_quads, 4, 2) in pixels of gray (NaN
// where not ok).  dict: uint16 (n_codes) or null.
int aruco_quads(const uint8_t* gray, int n, int h, int w, const int32_t* count, const int32_t* cand, int max_quads,
                const uint16_t* dict, int n_codes, int max_correction_bits, int border_errors, int32_t* ok,
                int32_t* ids, int32_t* rot, double* corners, hipStream_t s);

// the accepted quads of each image ordered by (id, label), the first max_markers of them: count int32 (n), ids int32
// (n, max_markers), corners float64 (n, max_markers, 4, 2) = p * ratio + (ratio - 1) / 2 per axis, NaN past the count
int aruco_collect(const int32_t* cand_count, const int32_t* cand, const int32_t* ok, const int32_t* ids,
                  const double* corners, int n, int max_quads, int max_markers, double ratio_x, double ratio_y,
                  int32_t* count_out, int32_t* ids_out, double* corners_out, hipStream_t s);

}  // namespace mq
