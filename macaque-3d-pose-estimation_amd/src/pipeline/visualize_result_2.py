"""visualize_result_2.proc mirror (reference src/pipeline/visualize_result_2.py): ``visualize_result.proc`` with
the second script's skeleton -- its longer limb list (draw_kps :98-127), no eye discs (:136-137), and the eyes set
to None by clean_kp (:39-41), so the limbs that end at an eye are not drawn either.  Everything else, the
deviations included, is src/pipeline/visualize_result.py's."""
from . import visualize_result as _v1

SKELETON = "v2"


def proc(data_name, i_cam, config_path, raw_data_dir=None, **kw):
    kw.setdefault("skeleton", SKELETON)
    return _v1.proc(data_name, i_cam, config_path, raw_data_dir, **kw)


if __name__ == '__main__':

    pass
