"""The case table of the conv geometry sweep (tests/conv_cases.py) can catch what it claims to catch - checked without a GPU:
every reference is integer-valued and small enough for exact fp32 accumulation, differs from each deliberately mistaken reference
its row names, has a tap in the padding (the few pad-free rows are listed), and only the over-wide rows break the two conditions
under which a row's first tap never moves backwards."""
import pytest
import torch

import conv_cases as cc

NAMES = [c["name"] for c in cc.CASES]
# geometries in which no tap ever leaves the image: a 1x1 with pad 0 (strided or not) has one tap, always inside; stride 2 with pad 0 and
# pad_end = 1 on 7x9 ends its last window at row 6 / column 8, so the extra zero row and column are never read
PAD_FREE = {"k1s2p0_8x8", "k1s2p0_7x5", "k1s2p0_8x8_c256", "k1s1p0_lda", "k1s1p0_lda_c256", "k3s2p0e1_7x9"}
OVER_WIDE = {"k3s1p2_4x6", "k1s1p1_4x6", "k3s1p2_3x5"}
KEYS = {"F", "T", "Hin", "Win", "KT", "KH", "KW", "stride", "pad", "pad_end", "ups", "Cin", "Co", "lda_extra"}


def test_table_shape():
    for c in cc.CASES:
        assert KEYS <= set(c) and c["catches"] and c["wrong"], c["name"]
        assert c["Cin"] in (64, 128, 256) and (c["Cin"] == 256) == c["name"].endswith("_c256") and c["F"] % c["T"] == 0
        Ho, Wo = cc.out_size(c)
        assert 1 <= c["F"] * Ho * Wo <= 700, c["name"]
        assert c["KT"] * c["KH"] * c["KW"] * c["Cin"] <= 9 * 256
    assert sum(c["Co"] == 72 for c in cc.CASES) == 1 and all(c["Co"] in (64, 72) or c.get("out_nchw") for c in cc.CASES)
    assert PAD_FREE | OVER_WIDE <= set(NAMES)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_reference_is_exact_in_fp32(name, wide):
    d = cc.reference(name, wide)
    c = d.case
    for t in (d.x, d.w, d.bias, d.conv, d.rows):
        assert torch.equal(t, t.round())
    assert d.x.abs().max() <= 4 and d.w.abs().max() <= 2 and d.bias.abs().max() <= 8
    assert d.rowbias is None or d.rowbias.abs().max() <= 8
    assert d.residual is None or d.residual.abs().max() <= 16
    # no partial sum, in any order, can exceed the sum of the magnitudes
    taps = c["KT"] * c["KH"] * c["KW"]
    assert taps * d.cin * 4 * 2 + 8 + 8 + 16 < 2 ** 24
    assert d.rows.abs().max() < 2 ** 24 and torch.equal(d.rows.float().double(), d.rows)
    assert d.x.shape == (c["F"] * c["Hin"] * c["Win"], cc.cin_of(c, wide)) and d.x_wide.shape[1] == d.cin + c["lda_extra"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_differs_from_the_mistakes_the_case_names(name):
    for wide in (False, True):
        d = cc.reference(name, wide)
        for mistake in d.case["wrong"]:
            wrong = cc.mistaken(d.case, d, mistake)
            right = cc.to_ncthw(d.case, d.conv).reshape(-1) if mistake == "nchw_T_ignored" else d.conv
            assert wrong.shape != right.shape or not torch.equal(wrong, right), f"{name}: the reference cannot tell `{mistake}` from the right answer"
            if mistake == "no_pad_end":           # the output is cropped: fewer rows
                assert wrong.shape[0] < right.shape[0]
            elif mistake != "pad_end_at_start":
                assert wrong.shape == right.shape, (name, mistake)


def test_every_mistake_is_used():
    used = {m for c in cc.CASES for m in c["wrong"]}
    assert used == {"no_pad_end", "pad_end_at_start", cc.NEIGHBOUR, "ups_shift", "ups_source_bounds", "stride_phase", "temporal_across_batch",
                    "temporal_edge_replicated", "lda_ignored", "nchw_T_ignored", "wrapped_rows_zero"}
    for c in cc.CASES:       # by kind: the mistake each family of geometries must tell apart
        if c["pad_end"] and c["name"] != "k3s2p0e1_7x9":
            assert "no_pad_end" in c["wrong"]
        if c["ups"] == 2 and c["Hin"] > 1:
            assert "ups_shift" in c["wrong"]
        if c["stride"] == 2 and c["Hin"] > 1:
            assert "stride_phase" in c["wrong"] or c["pad_end"]
        if c["KT"] == 3 and c["F"] > c["T"]:
            assert "temporal_across_batch" in c["wrong"]
        if c["KT"] == 1 and c["name"] not in PAD_FREE:
            assert cc.NEIGHBOUR in c["wrong"]


@pytest.mark.parametrize("name", NAMES)
def test_padding_taps_and_first_tap_order(name):
    c = cc.CASE_BY_NAME[name]
    n = cc.rows_with_an_out_of_image_tap(c)
    assert (n == 0) if name in PAD_FREE else (n > 0), n
    assert cc.first_tap_is_monotone(c) == (name not in OVER_WIDE)


def test_over_wide_rows_that_wrap():
    """Which tile heights hold a row whose first tap lies before the tile's first row's: none at 4x6 (see the table), the 128- and
    160-row tiles at 3x5 - there the model of the unsigned wrap changes the answer."""
    wrapped = {name: {bm: cc.conv_rows_wrapped(cc.CASE_BY_NAME[name], cc.reference(name, False).conv, bm)[1] for bm in (128, 160, 192, 256)}
               for name in sorted(OVER_WIDE)}
    assert not any(wrapped["k3s1p2_4x6"].values()) and not any(wrapped["k1s1p1_4x6"].values()), wrapped
    assert wrapped["k3s1p2_3x5"][128] > 0 and wrapped["k3s1p2_3x5"][160] > 0, wrapped      # hints 74 and 72
    for c in cc.CASES:
        if c["name"] not in OVER_WIDE and c["KT"] == 1 and c["ups"] == 1:
            assert not any(cc.conv_rows_wrapped(c, cc.reference(c["name"], False).conv, bm)[1] for bm in (128, 160, 192, 256)), c["name"]
