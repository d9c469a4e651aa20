"""Mirror of the reference's `utils` package for what the training scripts use on this path
(`from utils import *`, main_dca.py:11): the learning-rate schedule, the disparity metrics, the KITTI error map of
utils/visualization.py (with the colour-coded disparity map next to it) and `loss_disp_smoothness` (util.py:76-86, which the
reference defines and never calls)."""
from .experiment import adjust_learning_rate, learning_rate_adjust  # noqa: F401
from .metrics import D1_metric, EPE_metric, Thres_metric  # noqa: F401


def _package():
    """`dcanet_amd`, also when this directory is used as the top-level `utils` package (as models/_bootstrap.py does)"""
    import importlib.util
    import os
    import sys
    if "dcanet_amd" in sys.modules:
        return sys.modules["dcanet_amd"]
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models", "_bootstrap.py")
    spec = importlib.util.spec_from_file_location("_dca_bootstrap", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ensure()


from .visualization import (disp_error_image, disp_error_image_func, disp_to_color, error_colormap,  # noqa: E402,F401
                            gen_error_colormap)


def loss_disp_smoothness(disp, img):
    """reference util.py:76-86, same name and signature: the edge-aware smoothness of a (B,1,H,W) disparity map under a
    (B,C=3,H,W) image, sum |dd| exp(-mean_c |dI|) over all horizontal and vertical neighbour pairs divided by the sum of the
    weights.  It is the smoothness term of `ops.selfsup_loss` on its own (photometric weight 0: one forward and one
    backward launch of csrc/selfsup.hip, the second image is not read); ROCm tensors only, H >= 3 and W >= 3."""
    return _package().ops.selfsup_loss(img, img, [disp], (1.0,), None, lam=1.0, photo_scale=0.0)[0]
