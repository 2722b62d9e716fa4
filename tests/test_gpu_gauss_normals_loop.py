"""The normal-consistency demo (demo/NormalConsistency.py) as a test, at a size that takes seconds: flat oriented Gaussians on a
tilted plane, their quaternions fitted with 1 - n_rendered . n_depth through Renderer.gaussian_normals, get_rendered_normals,
get_depth and get_normals.  Both the loss and the mean angle between the Gaussians' normals and the plane's normal must fall; the
start and end values are logged, no ratio is fixed in advance."""
import importlib.util
import os

import numpy as np
import pytest

from util import log_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normal_consistency_demo_turns_the_gaussians_towards_the_plane(hip_lib):
    spec = importlib.util.spec_from_file_location("demo_NormalConsistency", os.path.join(ROOT, "demo", "NormalConsistency.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    out = demo.run(iters=60, size=64, side=12, K=8, log=lambda s: log_line("[demo] NormalConsistency: " + s))
    assert np.isfinite(out["loss"]).all() and np.isfinite(out["angle"]).all()
    assert 10.0 < out["angle"][0] < 35.0      # the start: tilts of 10 to 35 degrees
    assert out["loss"][-1] < out["loss"][0], (out["loss"][0], out["loss"][-1])
    assert out["angle"][-1] < out["angle"][0], (out["angle"][0], out["angle"][-1])
