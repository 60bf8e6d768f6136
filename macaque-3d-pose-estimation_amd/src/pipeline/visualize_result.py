"""visualize_result.proc mirror (reference src/pipeline/visualize_result.py:136-254): reproject kp3d into one
camera, draw every animal's skeleton over the camera's frames, and write the result.

The drawing runs on the GPU (``mqhip.overlay.OverlayRenderer``: ``mq_overlay_render``, csrc/overlay.hip).
Deviations from the reference, all stated in DESIGN.md section 8.5:

* where the reference writes ``<out>/<data>_<camid>.mp4`` (cv2 / ffmpeg, neither of which this build has), the
  default writes a frame store ``<out>/<data>_<camid>/`` that ``mqhip.io.FrameStore`` opens (``frames.npy`` uint8
  (N, H, W, 3) BGR, ``frame_number.npy``, ``frame_time.npy``, ``metadata.yaml``, empty ``tracks.json`` rows), and
  ``video='avi'`` writes a Motion-JPEG AVI ``<out>/<data>_<camid>.avi`` instead: the rendered frames are encoded
  on the GPU by the project's own baseline JPEG encoder (``mqhip.mjpeg.JpegEncoder``: ``mq_jpeg_encode``,
  csrc/jpeg.hip) and only the compressed streams leave the device (``mqhip.io.MjpegAviWriter``);
* the discs and limbs are covered by the project's own exact rules, not by cv2's fixed-point rasterisers, and the
  limb angle is not rounded to whole degrees: edges may differ from cv2's by a pixel;
* the cameras come from ``<result>/calibration.toml`` (what step 4 writes and reads), not from the h5 files.

Kept from the reference: ``kp3d_fxdJointLen.pickle`` is preferred over ``kp3d.pickle`` (:150-156), the "already
exists" (:146-148) and "no kp3d file" (:154-156) early returns, the frame lookup through
``<result>/<camid>/frame_num.npy`` (:172, :206), and a frame number absent from the store is skipped with a
warning (:209-211).
"""
import os

import numpy as np
import yaml

SKELETON = "v1"    # visualize_result.py's draw_kps; visualize_result_2 sets "v2"


def _gpu_renderer(cgroup, height, width, skeleton, mrksize, device):
    from mqhip.overlay import OverlayRenderer
    return OverlayRenderer(cgroup, height, width, skeleton=skeleton, mrksize=mrksize, device=device)


def _gpu_encoder(height, width, quality, device):
    from mqhip.mjpeg import JpegEncoder
    return JpegEncoder(height, width, quality=quality, device=device)


def _gpu_resizer(frames, height, width, device=0):
    from mqhip.resize import resize_bilinear
    return resize_bilinear(frames, height, width, device=device)


def proc(data_name, i_cam, config_path, raw_data_dir=None, results_dir_root='./results3D', out_dir='./output',
         device=0, batch=16, step=1, frame_range=None, skeleton=None, mrksize=3, renderer=None, video=None,
         quality=90, fps=24.0, encoder=None, decoder=None, size=None, resizer=None):
    """visualize_result.py:136-254 for camera ``camera_id[i_cam]`` of ``config_path``.

    ``step`` / ``frame_range=(start, stop)`` select the rows ``range(start, stop, step)`` of kp3d's frame axis
    (a full camera of the workload is 2.8 GB of frames); ``batch`` output images are rendered per launch, and
    the source images a batch needs are uploaded once (stores may keep a pool of images shared by many frames).
    ``renderer``: a factory ``(cgroup, height, width, skeleton, mrksize, device)`` of an object with
    ``OverlayRenderer.render``'s signature (tests inject the NumPy oracle); the default is the GPU renderer.
    ``video``: None (default) writes the frame store; ``'avi'`` encodes every rendered batch on the device at JPEG
    ``quality`` (the frames are not copied to the host) and writes ``<out>/<data>_<camid>.avi`` at ``fps`` with
    ``<out>/<data>_<camid>.frame_number.npy`` / ``.frame_time.npy`` beside it.  ``encoder``: a factory
    ``(height, width, quality=, device=)`` of an object with ``JpegEncoder.encode`` (tests inject the NumPy encoder).
    ``decoder``: the ``FrameStore``'s (a ``format: mjpeg`` store decodes on the GPU; with the GPU renderer the
    decoded batch never leaves the device).
    ``size``: None (default) keeps the camera's size; ``(width, height)`` resizes every rendered batch on the device
    before it is encoded or stored (``mqhip.resize.resize_bilinear``: the reference's cv2.resize to 800 x 600,
    :164, :249).  ``resizer``: a callable ``(frames, height, width, device=)`` in its place (tests inject NumPy).
    Returns the written store's directory (or the AVI's path), or None on the early returns."""
    from mqhip import io as mqio
    from mqhip.geometry import CameraGroup
    skeleton = SKELETON if skeleton is None else skeleton
    result_dir = os.path.join(results_dir_root, data_name)

    with open(config_path, 'r') as f:
        cfg = yaml.safe_load(f)
    ID = cfg['camera_id']

    if video not in (None, 'avi'):
        raise ValueError(f"video must be None or 'avi', got {video!r}")
    vid_path = os.path.join(out_dir, data_name + '_{:d}'.format(ID[i_cam]))
    if video == 'avi':
        vid_path += '.avi'

    if os.path.exists(vid_path if video == 'avi' else os.path.join(vid_path, 'metadata.yaml')):
        print('already exists:', vid_path)
        return None

    if os.path.exists(result_dir + '/kp3d_fxdJointLen.pickle'):
        kp3d_file = result_dir + '/kp3d_fxdJointLen.pickle'
    elif os.path.exists(result_dir + '/kp3d.pickle'):
        kp3d_file = result_dir + '/kp3d.pickle'
    else:
        print('no kp3d file:', data_name)
        return None

    print('generating...', vid_path)

    data = mqio.load_array_pickle(kp3d_file)
    data_name = os.path.basename(os.path.normpath(result_dir))
    mdata = raw_data_dir + '/' + data_name.split('.')[0] + '.' + str(ID[i_cam])
    frame_num = np.load(result_dir + '/' + str(ID[i_cam]) + '/frame_num.npy')
    store = mqio.FrameStore(mdata, decoder=decoder, device=device)
    store_frames_set = set(int(f) for f in store.get_frame_metadata()['frame_number'])

    X = np.asarray(data['kp3d'], dtype=np.float64)          # (A, F, J, 3)
    S = np.asarray(data['kp3d_score'], dtype=np.float64)    # (A, F, J)
    n_animal, n_frame, n_kp, _ = X.shape
    if len(frame_num) < n_frame:
        raise IndexError(f'{result_dir}/{ID[i_cam]}/frame_num.npy has {len(frame_num)} rows for {n_frame} frames')

    start, stop = (0, n_frame) if frame_range is None else frame_range
    rows = []                                               # (i_frame, frame number) of the frames to render
    for i_frame in range(max(0, int(start)), min(n_frame, int(stop)), max(1, int(step))):
        fn = int(frame_num[i_frame])
        if fn not in store_frames_set:
            print(f'[warning] Skipping frame {fn}: not found in the frame store')
            continue
        rows.append((i_frame, fn))

    H, W = (int(v) for v in store.frames.shape[1:3])
    cgroup = CameraGroup.load(result_dir + '/calibration.toml', device=device).subset_cameras_names([str(ID[i_cam])])
    draw = (renderer or _gpu_renderer)(cgroup, H, W, skeleton, mrksize, device)
    w_out, h_out = (W, H) if size is None else (int(size[0]), int(size[1]))
    if video == 'avi':
        encode = (encoder or _gpu_encoder)(h_out, w_out, quality=quality, device=device)
        writer = mqio.MjpegAviWriter(vid_path, h_out, w_out, fps=fps)
    else:
        writer = mqio.FrameStoreWriter(vid_path, len(rows), h_out, w_out, ID[i_cam])
    batch = max(1, int(batch))
    for k in range(0, len(rows), batch):
        part = rows[k:k + batch]
        idx = np.array([i for i, _ in part])
        fns = [fn for _, fn in part]
        pos = [store.index_of(fn) for fn in fns]
        pool, src_index = np.unique(store.frame_index[pos], return_inverse=True)
        if store.format == 'mjpeg' and renderer is None:     # decoded on the device: only JPEG bytes are uploaded
            frames = store.frames.device_frames([int(p) for p in pool], device)
        else:
            frames = np.stack([np.asarray(store.frames[int(p)]) for p in pool])      # each source image once
        out = draw.render(frames, 0, X[:, idx].transpose(1, 0, 2, 3), S[:, idx].transpose(1, 0, 2),
                          src_index=src_index.astype(np.int32))
        if size is not None:
            out = (resizer or _gpu_resizer)(out, h_out, w_out, device=device)
        if video == 'avi':
            for jpg, fn, t in zip(encode.encode(out), fns, store.frame_time[pos]):
                writer.append(jpg, fn, t)
            continue
        out = out.cpu().numpy() if hasattr(out, 'cpu') else np.asarray(out)
        writer.append(out, fns, store.frame_time[pos])
    writer.close()
    return vid_path


if __name__ == '__main__':

    pass
