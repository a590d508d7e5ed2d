"""Attention geometry sweep of geo4d_attention: every row of tests/attention_cases.py (text-only cross-attention with kv_div and column
slices, the resampler's 16 x 273, key counts around 1 / 8 / 64 / 128, two key/value sets, a segment switch with far-apart maxima) in
every mode, once per DISTINCT instantiation (kernel, nseg, qb, occ, ps) that ops.attention_plan resolves variants 0..5 to. Per launch:

  1. per-row parity: relative L2 per (batch, head, query row) against the float64 reference <= 2 x the project's attention tolerance
     (attention_cases.BOUND), where the older tests take one norm over the whole output;
  2. uniform attention (groups A-D): q = 0 and V from {-3, -1, 1, 3} make every P exactly 1 and l = Nk, so all query rows of a
     (batch, head) carry identical bits, within one unit in the last place (f32 outputs: two) of the mean of THAT key batch's V rows:
     a dropped, doubled or foreign key moves the sum by >= 1 (attention_cases.uniform_expected has the two-set tolerance);
  3. bit-for-bit independence of what the header says is never used: finite garbage in the V^T columns [Nk, next 16 bytes), NaN in
     the V^T columns up to the pitch, NaN in the K rows after the last key batch, NaN in the q rows after B * Nq;
  4. `out` is a column slice of a sentinel-filled buffer: nothing outside the [B * Nq, H * 64] window is written;
  5. the first and the last (batch, head), launched alone (B = 1, H = 1) on their own slices under the same variant, have the bits of
     the full launch (the second kernel's workgroup remap at workgroup counts that are no multiple of 8);
  6. two clean launches agree bit for bit;
  7. split_out (4-byte modes, one case per group): hi + lo of the pre-split output decode to the plain output.

The instantiations a test runs are the ones tests/test_attention_geometry_cpu.py counts: the real descriptor must resolve like the
CPU test's fake-pointer descriptor of the same (case, mode), so its proof that the table reaches all 20 builds at ragged shapes holds
for the launches made here.

Worst (batch, head, row) error measured on the MI355X over the whole table (460 (case, mode, build) runs, all 20 instantiations), per mode:
  mode       worst row   bound     where
  f32        9.2e-06     4e-05     E_far_maxima, two-set build (groups A-D: 9.0e-07)
  bf16       3.9e-03     1.2e-02   A_nq128, first kernel with two query blocks per wave
  f16        4.7e-04     2e-03     A_nq256, second kernel
  bf16x3     2.7e-05     1e-04     E_far_maxima, two-set build (groups A-D: 1.6e-05)
  bf16x3ps   1.6e-05     1e-04     A_nk80_nq300, second kernel at one wave per SIMD"""
import ctypes

import pytest
import torch

import attention_cases as ac
from test_presplit_gpu import check_split

pytestmark = pytest.mark.gpu


def _kw(mode):
    return dict(x3=mode == "bf16x3", qkv_split=mode == "bf16x3ps")


def _run(dev, mode, qv, kv, B, Hh, Nq, variant):
    """One launch into a guarded output (check 4); returns a contiguous copy of the window."""
    from geo4d_amd import ops
    rows, cols = B * Nq, Hh * 64
    odt = torch.float32 if ac.four_byte(mode) else ac.torch_dtype(mode)
    buf = torch.full((rows + ac.EXTRA_ROWS, cols + 2 * ac.OUT_PAD), ac.SENTINEL, dtype=odt, device=dev)
    out = buf[:rows, ac.OUT_PAD:ac.OUT_PAD + cols]
    assert out.data_ptr() % 16 == 0
    ops.attention(qv, kv, B=B, H=Hh, Nq=Nq, scale=ac.SCALE, out=out, variant=variant, **_kw(mode))
    res = out.clone()
    out.fill_(ac.SENTINEL)
    assert (buf == ac.SENTINEL).all(), "the launch wrote outside its [B*Nq, H*64] output window"
    return res


@pytest.mark.parametrize("name,mode", ac.case_modes())
def test_attention_geometry(dev, name, mode):
    from geo4d_amd import ops
    from geo4d_amd._lib import AttentionPlan, check, load
    case = ac.BY_NAME[name]
    B, Nq = case["B"], case["Nq"]
    q, sets = ac.make_data(name, mode)
    ref = ac.reference(q, sets, B, ac.H, Nq, ac.SCALE)
    qv, kv, bufs = ac.launch_args(case, mode, q, sets, dev)
    poisoned = {p: ac.launch_args(case, mode, q, sets, dev, poison=(p,))[:2] for p in ac.poisons_of(case, mode)}
    uniform = case["group"] != "E"
    if uniform:
        uq, usets = ac.make_data(name, mode, uniform=True)
        uqv, ukv, _ = ac.launch_args(case, mode, uq, usets, dev)
        exact, tol = ac.uniform_expected(usets, B, mode)

    def plan_of(variant):
        return ops.attention_plan(ops.attention_descriptor(qv, kv, B=B, H=ac.H, Nq=Nq, scale=ac.SCALE, variant=variant, **_kw(mode))[0])

    def fake_plan_of(variant):
        plan = AttentionPlan()
        check(load().geo4d_attention_plan(ctypes.byref(ac.fake_descriptor(case, mode, variant)), ctypes.byref(plan)), "geo4d_attention_plan")
        return plan

    insts = ac.instantiations(case, mode, plan_of)
    assert insts, "the planner refused every variant"
    assert [i[:2] for i in insts] == [i[:2] for i in ac.instantiations(case, mode, fake_plan_of)], "the real descriptor resolves unlike the CPU test's"
    for variant, key, plan in insts:
        tag = f"{name} {mode} {key} variant {variant}"
        out = _run(dev, mode, qv, kv, B, ac.H, Nq, variant)
        # 1. per-row parity
        worst, glob = ac.row_err(out.cpu(), ref)
        print(f"[attn-geo] {tag}: worst row {worst:.3e}, global {glob:.3e}, bound {ac.BOUND[mode]:.1e}")
        assert worst <= ac.BOUND[mode], tag
        # 6. determinism
        assert torch.equal(out, _run(dev, mode, qv, kv, B, ac.H, Nq, variant)), tag
        # 3. padding and neighbour independence
        for p, (pq, pkv) in poisoned.items():
            assert torch.equal(out, _run(dev, mode, pq, pkv, B, ac.H, Nq, variant)), f"{tag}: poison ({p}) changed the output"
        # 5. isolation of the first and the last (batch, head)
        for b, h in ((0, 0), (B - 1, ac.H - 1)):
            iq, ikv = ac.isolated_args(case, mode, bufs, b, h)
            alone = _run(dev, mode, iq, ikv, 1, 1, Nq, plan.variant)
            assert torch.equal(alone, out[b * Nq:(b + 1) * Nq, 64 * h:64 * (h + 1)]), f"{tag}: (batch {b}, head {h}) alone differs"
        # 2. uniform attention
        if uniform:
            u = _run(dev, mode, uqv, ukv, B, ac.H, Nq, variant).cpu().double().reshape(B, Nq, ac.C)
            assert torch.equal(u, u[:, :1].expand_as(u)), f"{tag}: query rows of one (batch, head) differ under uniform attention"
            over = ((u[:, 0] - exact).abs() - tol).max().item()
            assert over <= 0, f"{tag}: uniform attention is not the mean of the key batch's values (over by {over:.3e})"
        # 7. split_out
        if name in ac.SPLIT_OUT_CASES and ac.four_byte(mode):
            so = ops.attention(qv, kv, B=B, H=ac.H, Nq=Nq, scale=ac.SCALE, variant=variant, split_out=True, **_kw(mode))
            assert isinstance(so, ops.SplitAct)
            check_split(tag, so, out)
