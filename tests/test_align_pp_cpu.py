"""Principal points in the global alignment, the parts that need no GPU: the new C entry points in the header, the ctypes table and the
built library; the untouched ABI; the committed fixture; argument errors raised before any device work."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("geo4d_align_pp_workspace", "geo4d_align_residual_pp", "geo4d_align_set_pp", "geo4d_align_pp_grads")


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from geo4d_amd import _lib
    with open(os.path.join(ROOT, "include", "geo4d_hip.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(geo4d_[a-z_0-9]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["geo4d_align_residual_pp"][1][0]._type_ is _lib.Align         # the existing descriptor, not a new struct
    assert lib.geo4d_align_pp_workspace(7, 16, 12, 16, 256) == lib.geo4d_align_workspace(7, 16, 12, 16, 256) + 7 * 1 * 2 * 4
    assert lib.geo4d_align_pp_workspace(5, 8, 40, 64, 1024) == lib.geo4d_align_workspace(5, 8, 40, 64, 1024) + 5 * 3 * 2 * 4
    assert lib.geo4d_align_pp_workspace(0, 8, 40, 64, 1024) == 0
    # argument validation on the host, before any launch
    a = _lib.Align()
    assert lib.geo4d_align_residual_pp(ctypes.byref(a), None, None) == -22 and b"align_residual_pp" in lib.geo4d_last_error()
    assert lib.geo4d_align_set_pp(None, None, 3, 8.0, 6.0, None) == -22 and b"align_set_pp" in lib.geo4d_last_error()
    assert lib.geo4d_align_pp_grads(None, None, 3, None) == -22 and b"align_pp_grads" in lib.geo4d_last_error()


def test_abi_version_and_struct_sizes_are_unchanged():
    from geo4d_amd import _lib
    with open(os.path.join(ROOT, "include", "geo4d_hip.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define GEO4D_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9     # symbols added, no struct changed
    lib = _lib.load()
    assert lib.geo4d_abi_version() == 9
    # sizeof of every parameter struct as ABI 9 shipped it (LP64): conv_gemm, groupnorm, attention, align, align_small
    sizes = [lib.geo4d_abi_struct_size(k) for k in range(5)]
    assert sizes == [ctypes.sizeof(s) for s in (_lib.ConvGemm, _lib.GroupNorm, _lib.Attention, _lib.Align, _lib.AlignSmall)]
    assert sizes[0] == 9 * 8 + 9 * 8 + 27 * 4 + 4 + 3 * 4 + 4 + 8 + 8
    assert sizes[3] == 16 * 8 + 6 * 4 + 3 * 4 + 4 and sizes[4] == 28 * 8 + 7 * 4 + 7 * 4
    assert lib.geo4d_abi_struct_size(5) == 0


def test_fixture_loads_and_its_preset_case_keeps_the_preset():
    g = torch.load(os.path.join(ROOT, "tests", "golden", "align_pp_tiny.pt"), weights_only=False)
    base = torch.load(os.path.join(ROOT, "tests", "golden", "align_tiny.pt"), weights_only=False)
    H, W = base["pred"].shape[2:4]
    n = 1 + max(max(grp) for grp in base["groups"])
    assert g["niter"] == 40 and g["lr"] == 0.03 and g["lr_min"] == 1e-3 and g["schedule"] == "linear"
    want = (g["preset_pixels"] - torch.tensor([W / 2, H / 2])) / 10
    assert g["preset_pixels"].shape == (n, 2) and len({tuple(r) for r in g["preset_pixels"].tolist()}) == n     # differ between images
    assert torch.allclose(g["preset"]["init"]["im_pp"], want, atol=1e-7)
    assert torch.equal(g["preset"]["after"]["im_pp"], g["preset"]["init"]["im_pp"])
    assert "im_pp" not in g["preset"]["grads"] and set(g["preset"]["grads"]) == {"im_depthmaps", "im_poses", "im_focals", "pw_poses"}
    for case in ("optimize", "per_image"):
        assert set(g[case]["grads"]) == {"im_depthmaps", "im_poses", "im_focals", "pw_poses", "im_pp"}
        assert g[case]["grads"]["im_pp"].shape == (n, 2) and float(g[case]["grads"]["im_pp"].norm()) > 0
    assert g["per_image"]["init"]["im_focals"].shape == (n, 1)
    # the shared start is align_tiny.pt's seeded start plus im_pp
    for k, v in base["init"].items():
        assert torch.equal(g["optimize"]["init"][k], v), k
    assert torch.equal(g["optimize"]["init"]["im_pp"], g["im_pp0"])
    assert not torch.equal(g["optimize"]["after"]["im_pp"], g["im_pp0"])
    assert set(g["fp64"]["rel"]) == set(g["optimize"]["after"]) and all(0 <= v < 1e-3 for v in g["fp64"]["rel"].values())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "align_pp_tiny.pt")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "align_tiny.pt"))


def test_post_optimization_argument_errors_come_before_any_device_work():
    """CPU tensors: anything past the argument checks would raise Geo4DNativeError (no CPU path), so a ValueError proves the order."""
    from geo4d_amd.align import post_optimization
    from geo4d_amd.pipeline import window_slices
    T, H, W, n = 4, 16, 24, 7
    slices = window_slices(n, 1, T)
    maps, traj = torch.zeros(len(slices), 11, T, H, W), torch.eye(4).repeat(len(slices), T, 1, 1)
    K = torch.eye(3).repeat(n, 1, 1)
    with pytest.raises(ValueError, match=r"principal_points: expected \[7, 2\]"):
        post_optimization(slices, maps, traj, principal_points=torch.zeros(n, 3))
    with pytest.raises(ValueError, match=r"principal_points: expected \[7, 2\]"):
        post_optimization(slices, maps, traj, principal_points=torch.zeros(n - 1, 2), intrinsics=K)
    with pytest.raises(ValueError, match="needs intrinsics"):
        post_optimization(slices, maps, traj, principal_points="intrinsics")
    with pytest.raises(ValueError, match="or 'intrinsics'"):
        post_optimization(slices, maps, traj, principal_points="centre", intrinsics=K)
