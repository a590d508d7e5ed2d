"""The attention geometry sweep (tests/attention_cases.py) checked without a GPU:
  * `reference` is torch's scaled_dot_product_attention in float64 (keys repeated kv_div times; two sets: the sum of two calls);
  * resolved through geo4d_attention_plan (host code), the table reaches exactly the 20 built instantiations, each of them with a
    ragged last key tile and with a partly empty workgroup, the second kernel's four also with kv_div > 1 and with fewer than 64 keys;
  * the kernels' rounding points alone (`emulate`) stay within a third of the per-row bound the GPU test applies
    (tests/test_attention_geometry_gpu.py), so that bound leaves the schedule (lazy rescale, summation order) two thirds of itself."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

import attention_cases as ac

F32, BF16, F16, BF16X3 = 0, 1, 2, 3
# (dtype, kernel, nseg, qb, occ, ps): the 20 instantiations of ATTN_INSTANCES, as tests/test_attention_plan_cpu.py lists them
FIRST = {(d, 1) + i + (0,) for d in range(4) for i in ((2, 1, 1), (1, 2, 2), (1, 1, 1))} | {(d, 1, 1, 1, 4, 0) for d in (BF16, F16)} | \
        {(BF16X3, 1, 1, 2, 2, 1), (BF16X3, 1, 1, 1, 1, 1)}
SECOND = {(BF16, 2, 1, 2, 2, 0), (F16, 2, 1, 2, 2, 0), (BF16X3, 2, 1, 2, 1, 1), (BF16X3, 2, 1, 2, 2, 1)}


def _sdpa64(q, k, v, nk, div, B, Nq):
    heads = lambda x, b, n: x.double().reshape(b, n, ac.H, 64).permute(0, 2, 1, 3)
    o = TF.scaled_dot_product_attention(heads(q, B, Nq), heads(k, B // div, nk).repeat_interleave(div, 0),
                                        heads(v, B // div, nk).repeat_interleave(div, 0), scale=ac.SCALE)
    return o.permute(0, 2, 1, 3).reshape(B * Nq, ac.C)


@pytest.mark.parametrize("name", [c["name"] for c in ac.CASES if "f32" in ac.modes_of(c)])
def test_reference_is_sdpa_in_float64(name):
    c = ac.BY_NAME[name]
    q, sets = ac.make_data(name, "f32")
    ref = ac.reference(q, sets, c["B"], ac.H, c["Nq"], ac.SCALE)
    want = sum(_sdpa64(q, k, v, nk, div, c["B"], c["Nq"]) for k, v, nk, div in sets)
    assert ref.dtype == torch.float64 and ref.shape == (c["B"] * c["Nq"], ac.C)
    assert (ref - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_the_table_reaches_every_instantiation_at_ragged_shapes():
    from geo4d_amd import _lib
    lib = _lib.load()

    def plan_of(case, mode):
        def ask(variant):
            plan = _lib.AttentionPlan()
            _lib.check(lib.geo4d_attention_plan(ctypes.byref(ac.fake_descriptor(case, mode, variant)), ctypes.byref(plan)), "geo4d_attention_plan")
            return plan
        return ask

    hit, ragged_nk, ragged_nq, div_gt1, nk_lt64 = {}, {}, {}, {}, {}
    for name, mode in ac.case_modes():
        case = ac.BY_NAME[name]
        for variant, key, plan in ac.instantiations(case, mode, plan_of(case, mode)):
            inst = (ac.DTYPE_CODE[mode],) + key
            assert plan.rows_per_wg == 128 * plan.qb
            hit.setdefault(inst, name)
            if any(nk % 64 for nk, _ in case["sets"]):
                ragged_nk.setdefault(inst, name)
            if case["Nq"] % plan.rows_per_wg:
                ragged_nq.setdefault(inst, name)
            if any(div > 1 for _, div in case["sets"]):
                div_gt1.setdefault(inst, name)
            if any(nk < 64 for nk, _ in case["sets"]):
                nk_lt64.setdefault(inst, name)
    for inst in sorted(FIRST | SECOND):
        print(f"[attn-geo] {inst}: ragged Nk {ragged_nk.get(inst)}, ragged Nq {ragged_nq.get(inst)}, kv_div > 1 {div_gt1.get(inst)}, Nk < 64 {nk_lt64.get(inst)}")
    assert set(hit) == FIRST | SECOND and len(hit) == 20
    assert set(ragged_nk) == set(hit), sorted(set(hit) - set(ragged_nk))
    assert set(ragged_nq) == set(hit), sorted(set(hit) - set(ragged_nq))
    assert SECOND <= set(div_gt1) and SECOND <= set(nk_lt64)


@pytest.mark.parametrize("name,mode", ac.case_modes())
def test_rounding_points_alone_stay_within_a_third_of_the_bound(name, mode):
    c = ac.BY_NAME[name]
    q, sets = ac.make_data(name, mode)
    ref = ac.reference(q, sets, c["B"], ac.H, c["Nq"], ac.SCALE)
    worst, glob = ac.row_err(ac.emulate(q, sets, c["B"], ac.H, c["Nq"], ac.SCALE, mode), ref)
    print(f"[attn-geo] {name} {mode}: emulated worst row {worst:.3e}, global {glob:.3e}, bound {ac.BOUND[mode]:.1e}")
    assert worst <= ac.BOUND[mode] / 3


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in ac.case_modes() if ac.BY_NAME[n]["group"] != "E"])
def test_emulated_uniform_attention_is_the_mean_of_the_values(name, mode):
    """The uniform-attention check of the GPU test on the emulation: q = 0 gives every row the mean of its key batch's V rows to the
    last place, so the tolerance of that check is one the arithmetic meets."""
    c = ac.BY_NAME[name]
    q, sets = ac.make_data(name, mode, uniform=True)
    out = ac.emulate(q, sets, c["B"], ac.H, c["Nq"], ac.SCALE, mode).double().reshape(c["B"], c["Nq"], ac.C)
    exact, tol = ac.uniform_expected(sets, c["B"], mode)
    assert torch.equal(out, out[:, :1].expand_as(out))
    assert ((out[:, 0] - exact).abs() <= tol).all()
