"""geo4d_amd/scene_view.py without a GPU and without the library: what scene_view does to a scene and in which order, on a duck-typed
scene that records the calls made on it (n = 2, H = 3, W = 4, CPU tensors); voxel_option and MeshOptions against the expressions and
checks they replace; and the import graph of the scene layer."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from geo4d_amd import mesh
from geo4d_amd.scene_view import MOTION, MeshOptions, SceneView, scene_view, voxel_option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 3, 4
THR = dict(min_conf_thr=1.5, thr_for_init_conf=False, is_msk=True)
GETTERS = ("get_pts3d", "get_depthmaps", "get_focals", "get_conf", "get_im_poses_matrix", "get_principal_points")


class Scene:
    """A GroupAligner as far as scene_view knows one. `calls` lists, in order, every method called, every attribute set (as
    ("set", name, value)) and every read of `imgs`."""
    n, H, W, dev = N, H, W, torch.device("cpu")

    def __init__(self, imgs=True, dynamic_masks=None, complete=True):
        self.__dict__.update(calls=[], complete=complete, min_conf_thr=None, thr_for_init_conf=None, dynamic_masks=dynamic_masks,
                             _imgs=torch.rand(N, H, W, 3, dtype=torch.float64) if imgs else None,
                             conf=torch.arange(N * H * W, dtype=torch.float32).reshape(N, H, W) / 8)

    def __setattr__(self, name, value):
        self.calls.append(("set", name, value))
        self.__dict__[name] = value

    @property
    def imgs(self):
        self.calls.append("imgs")
        return self._imgs

    def require_all_depthmaps(self, who):
        self.calls.append(("require_all_depthmaps", who))
        if not self.complete:
            raise RuntimeError(f"{who} needs every image's depth map")

    def get_masks(self):
        self.calls.append("get_masks")
        assert self.thr_for_init_conf is False                      # the thresholds are on the scene by now
        return self.conf > self.min_conf_thr

    def _tensor(self, name, *shape):
        self.calls.append(name)
        return torch.ones(shape).requires_grad_()

    get_pts3d = lambda self: self._tensor("get_pts3d", N, H, W, 3)
    get_depthmaps = lambda self: self._tensor("get_depthmaps", N, W, H).transpose(1, 2)       # not contiguous
    get_focals = lambda self: self._tensor("get_focals", N, 1)
    get_conf = lambda self: self._tensor("get_conf", N, H, W)
    get_principal_points = lambda self: self._tensor("get_principal_points", N, 2)
    get_im_poses_matrix = lambda self: self._tensor("get_im_poses_matrix", N, 4, 4)


def _dyn():
    return (torch.arange(N * H * W).reshape(N, H, W) % 3) == 0


def _never(*a, **kw):
    raise AssertionError("segment_motion must not be called here")


def test_construction_order_and_nothing_more():
    s = Scene()
    view = scene_view(s, "caller", **THR)
    assert isinstance(view, SceneView)
    assert s.calls == [("require_all_depthmaps", "caller"), ("set", "min_conf_thr", 1.5), ("set", "thr_for_init_conf", False), "get_masks"]
    assert torch.equal(view.msk, s.conf > 1.5) and 0 < int(view.msk.sum()) < N * H * W
    assert (view.n, view.H, view.W, view.dev) == (N, H, W, s.dev)
    assert view.thresholds == THR
    # a scene that lacks depth maps is refused in the caller's name before anything is set or read
    s = Scene(complete=False)
    with pytest.raises(RuntimeError, match="^caller needs every image's depth map"):
        scene_view(s, "caller", **THR)
    assert s.calls == [("require_all_depthmaps", "caller")] and s.min_conf_thr is None


def test_is_msk_false_takes_no_mask():
    s = Scene()
    view = scene_view(s, "caller", **dict(THR, is_msk=False))
    assert view.msk is None and "get_masks" not in s.calls
    assert [c for c in s.calls if c[0] == "set"] == [("set", "min_conf_thr", 1.5), ("set", "thr_for_init_conf", False)]
    assert view.mask() is None


def test_tensors_are_read_on_demand_once_detached_and_contiguous():
    s = Scene()
    view = scene_view(s, "caller", **THR)
    assert not set(GETTERS) & set(s.calls)
    for name, getter, shape in (("pts3d", "get_pts3d", (N, H, W, 3)), ("depth", "get_depthmaps", (N, H, W)), ("focals", "get_focals", (N, 1)),
                                ("conf", "get_conf", (N, H, W)), ("poses", "get_im_poses_matrix", (N, 4, 4))):
        before = list(s.calls)
        t = getattr(view, name)
        assert s.calls == before + [getter], name                   # this getter and no other
        assert getattr(view, name) is t and s.calls == before + [getter], name
        assert tuple(t.shape) == shape and not t.requires_grad, name
    assert view.pts3d.is_contiguous() and view.depth.is_contiguous() and not s.get_depthmaps().is_contiguous()
    before = list(s.calls)
    c2w, K = view.cameras
    assert sorted(s.calls[len(before):]) == ["get_focals", "get_im_poses_matrix", "get_principal_points"]
    assert c2w.dtype == K.dtype == torch.float64 and tuple(c2w.shape) == (N, 4, 4) and tuple(K.shape) == (N, 3, 3)
    assert torch.equal(K[0], torch.tensor([[1, 0, 1], [0, 1, 1], [0, 0, 1]], dtype=torch.float64))
    assert view.cameras[0] is c2w
    assert "imgs" not in s.calls                                    # nothing but `rgb` / `imgs` touches scene.imgs


@pytest.mark.parametrize("is_msk", [True, False])
def test_mask_restricts_by_the_scenes_dynamic_masks(is_msk):
    dyn = _dyn()
    s = Scene(dynamic_masks=dyn)
    view = scene_view(s, "caller", **dict(THR, is_msk=is_msk), segment=_never)
    msk = s.conf > 1.5
    assert view.dynamic() is dyn
    assert torch.equal(view.mask("static"), msk & ~dyn if is_msk else ~dyn)
    assert torch.equal(view.mask("dynamic"), msk & dyn if is_msk else dyn)
    assert view.mask(None) is view.msk and view.mask() is view.msk
    for motion in MOTION:                                           # the view's own part is the default
        own = scene_view(s, "caller", **dict(THR, is_msk=is_msk), motion=motion, segment=_never)
        expect = view.mask(motion)
        assert own.mask() is None if expect is None else torch.equal(own.mask(), expect), motion
    assert "imgs" not in s.calls and not set(GETTERS) & set(s.calls)


def test_dynamic_segments_with_the_views_thresholds_when_the_scene_has_no_masks():
    s, seen = Scene(), []

    def segment(scene, **kw):
        seen.append((scene, kw))
        scene.dynamic_masks = _dyn()                                # as segment_motion leaves them
        return scene.dynamic_masks

    view = scene_view(s, "caller", **THR, segment=segment)
    assert seen == []                                               # not before somebody asks
    assert torch.equal(view.mask("dynamic"), (s.conf > 1.5) & _dyn())
    assert seen == [(s, THR)]
    assert torch.equal(view.dynamic(), _dyn()) and len(seen) == 1   # the scene has them now


def test_imgs_raises_in_the_callers_name_and_rgb_does_not():
    s = Scene(imgs=False)
    view = scene_view(s, "caller", **THR)
    assert "imgs" not in s.calls
    assert view.rgb is None
    with pytest.raises(ValueError, match=r"^caller: the scene has no RGB frames; pass imgs= to post_optimization or set scene.imgs "
                                         r"\[n, H, W, 3\] in \[0, 1\]$"):
        view.imgs
    s = Scene()
    view = scene_view(s, "caller", **THR)
    assert view.imgs is view.rgb and view.imgs.dtype == torch.float32 and view.imgs.is_contiguous()
    assert torch.equal(view.imgs, s._imgs.float())


def test_voxel_option():
    for x in (None, False):
        assert voxel_option(x) == (False, None)
    assert voxel_option(True) == (True, None)
    assert voxel_option(0.05) == (True, 0.05)
    on, voxel = voxel_option(np.float32(0.05))
    assert on is True and type(voxel) is np.float32 and voxel == np.float32(0.05)
    for x in (None, False, True, 0.05, np.float32(0.05), 1, 0.0):    # the expressions of the call sites this replaces
        on, voxel = voxel_option(x)
        assert on is (x is not None and x is not False), x
        if on:
            assert voxel is (None if x is True else x), x


def _message(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except ValueError as e:
        return str(e)
    return None


def test_mesh_options():
    assert MeshOptions() == MeshOptions(None, None, None, True, False)
    assert not MeshOptions().filtering and not MeshOptions().shaping
    assert vars(MeshOptions(3, 0.5, 2, False, True)) == dict(min_component_faces=3, min_component_fraction=0.5, smooth_iterations=2,
                                                             smooth_pin_boundary=False, normals=True)
    for faces in (None, 3):
        for fraction in (None, 0.5):
            for iterations in (None, 0, 2):
                for pin in (True, False):
                    for normals in (False, True):
                        o = MeshOptions(faces, fraction, iterations, pin, normals)
                        assert o.filtering is (faces is not None or fraction is not None)
                        assert o.shaping is bool(iterations is not None or pin is not True or normals)
                        o.check("x")                                # all of these are valid
    for kw in (dict(min_component_faces=0), dict(min_component_faces=2.5), dict(min_component_faces=True), dict(min_component_fraction=0.0),
               dict(min_component_fraction=2), dict(min_component_fraction="half")):
        want = _message(mesh.check_keep_args, kw.get("min_component_faces"), kw.get("min_component_fraction"), who="x")
        assert want is not None and want.startswith("x: ") and _message(MeshOptions(**kw).check, "x") == want, kw
    for iterations in (-2, 1.5, True, "3"):
        want = _message(mesh.check_smooth_args, iterations, who="x")
        assert want is not None and want.startswith("x: ") and _message(MeshOptions(smooth_iterations=iterations).check, "x") == want
    assert _message(MeshOptions(0, None, -1).check, "x") == _message(mesh.check_keep_args, 0, None, who="x")   # the filter's check first


# ---- the import graph ------------------------------------------------------------------------------------------------------------------
LAYER = ("scene_view", "motion", "fusion", "tsdf", "render", "scene_export")             # each imports only from those before it, and mesh
LAZY = {("scene_export", "camera_colors", "matplotlib"), ("render", "save_render", "PIL"), ("scene_export", "save_scene", "align")}


def _imports(node):
    """(level, module) of the import statements below `node`."""
    for n in ast.walk(node):
        if isinstance(n, ast.ImportFrom):
            yield from ((n.level, n.module or a.name) for a in n.names)
        elif isinstance(n, ast.Import):
            yield from ((0, a.name) for a in n.names)


def test_the_scene_layer_imports_at_module_scope_and_without_cycles():
    for name in LAYER + ("mesh",):
        tree = ast.parse(open(os.path.join(ROOT, "geo4d_amd", name + ".py")).read())
        inside = set()
        for fn in (n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda))):
            inside |= {(name, getattr(fn, "name", "lambda"), module.split(".")[0]) for _, module in _imports(fn)}
        assert inside <= LAZY, (name, inside - LAZY)
        below = set(LAYER[:LAYER.index(name)]) if name in LAYER else set()
        allowed = (below | {"mesh", "_lib", "ops", "io"}) - {name}
        top = {module.split(".")[0] for stmt in tree.body for level, module in _imports(stmt) if level and not isinstance(stmt, ast.FunctionDef)}
        assert top <= allowed, (name, top - allowed)


def test_scene_export_imports_in_a_fresh_interpreter():
    done = subprocess.run([sys.executable, "-c", "import geo4d_amd.scene_export, geo4d_amd.align"], cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
