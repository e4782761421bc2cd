"""CPU: the encoder's kernel-form table, pinned through `nlsh_encode_form` -- the plan `nlsh_encode_hash` itself
runs, read back without a launch -- at every boundary of the table: row counts, hidden and input widths, probe counts, and the room
each form's LDS image leaves for the epilogue's tables.  No device is needed: the HET expectations use the CU count the call reports."""
import pytest

import encoder_form_cases as fc
from encoder_form_cases import BUILD128, H16, HET, PINGPONG, SINGLE, SINGLE_WIDE
from nlsh_amd import _capi

NARROW = [128, 256, 256, 16]       # hidden layers of exactly 256: the widest the one-tile-per-wave forms take
ROWS = {H16: 16, SINGLE: 32, SINGLE_WIDE: 32, BUILD128: 128, PINGPONG: 64, HET: 32}


def plan(n, dims, n_probes=1):
    form, rows, lds, cus = _capi.encode_form(n, dims, n_probes)
    assert rows == ROWS[form], (n, dims, form, rows)
    assert 0 < lds <= fc.LDS_LIMIT, (n, dims, n_probes, lds)
    assert cus >= 1
    return form, rows, lds, cus


def single_or_het(n, cus):
    """The table's rows for the 32-row forms of a narrow encoder: HET when the rows behind the last full round of workgroups are at
    most half a round."""
    R = 32 * cus
    return HET if n > R and 0 < n % R <= R // 2 else SINGLE


def narrow_form(n, cus, build128=True):
    """Expected form of an encoder with hidden widths <= 256 (`build128`: its image also fits at 128 rows)."""
    if n <= 4096:
        return H16
    if n > 16384 and build128:
        return BUILD128
    return single_or_het(n, cus)


def test_row_count_boundaries():
    cus = fc.cus()
    R = 32 * cus
    assert plan(1, NARROW)[0] == H16 and plan(4096, NARROW)[0] == H16
    assert plan(4097, NARROW)[0] == narrow_form(4097, cus) != H16
    assert plan(16384, NARROW)[0] == narrow_form(16384, cus) != BUILD128
    assert plan(16385, NARROW)[0] == BUILD128
    for n in (R, R + 1, R + R // 2, R + R // 2 + 1, 2 * R, 2 * R + 1):
        assert plan(n, NARROW)[0] == narrow_form(n, cus), n
    # an input too wide for the 128-row image keeps the 32-row forms at every n, so the HET rule is visible on any CU count
    wide_in = [320, 64, 8]
    for n in (R, R + 1, R + R // 2, R + R // 2 + 1, 2 * R, 2 * R + 1, 2 * R + R // 2, 2 * R + R // 2 + 1):
        if n > 4096:
            assert plan(n, wide_in)[0] == single_or_het(n, cus), n
    big = [n for n in (R + 1, R + R // 2, R + R // 2 + 1) if n > 4096]
    if big:
        assert [plan(n, wide_in)[0] for n in big] == [HET, HET, SINGLE][-len(big):]
    # rows per workgroup and the LDS image follow the form: the same row stride at 16, 32 and 128 rows
    s = {n: fc.row_stride(*plan(n, NARROW)[:3]) for n in (130, 4097, 16385)}
    assert s[130] == s[4097] == s[16385] == 256 + 4


def test_hidden_width_boundaries():
    cus = fc.cus()
    for n, at256, at257 in ((130, H16, SINGLE_WIDE), (4097, narrow_form(4097, cus), SINGLE_WIDE), (16385, BUILD128, PINGPONG)):
        assert plan(n, [128, 256, 16])[0] == at256, n
        assert plan(n, [128, 257, 16])[0] == at257, n
        assert plan(n, [128, 64, 257, 64, 16])[0] == at257, n          # the WIDEST hidden layer decides, wherever it sits
    # two 64-row images fit up to a padded width of 312
    assert plan(16385, [128, 312, 16])[0] == PINGPONG
    assert plan(16385, [128, 313, 16])[0] == SINGLE_WIDE
    assert plan(20000, [128, 632, 632, 16])[0] == SINGLE_WIDE
    assert fc.row_stride(*plan(16385, [128, 312, 16])[:3]) == 316


def test_input_width_boundaries_above_16384_rows():
    cus = fc.cus()
    for n in (16385, 20000):
        assert plan(n, [312, 256, 16])[0] == BUILD128
        assert plan(n, [313, 256, 16])[0] == single_or_het(n, cus)
        assert plan(n, [312, 300, 16])[0] == PINGPONG
        assert plan(n, [313, 300, 16])[0] == SINGLE_WIDE
    form, rows, lds, _ = plan(20000, [1024, 64, 7])                       # the widest input: a 32-row form, not a refusal
    assert form == single_or_het(20000, cus) and rows == 32 and lds == 32 * (1024 + 4) * 4


@pytest.mark.parametrize("n,rows", [(130, 16), (4097, 32), (16385, 128)])
def test_probe_count_sizes_the_row_stride_of_a_narrow_encoder(n, rows):
    """Hidden width 32: the row stride comes from the epilogue's tables, 72 + n_probes rounded up to 8, + 4."""
    for n_probes, S in ((1, 84), (64, 140), (65, 148), (128, 204)):
        form, r, lds, _ = plan(n, [25, 32, 8], n_probes)
        assert r == rows and lds == rows * S * 4, (n_probes, lds)
        assert fc.row_stride(form, r, lds) == S
    # two images: z, p and the key table do not sit side by side there, so the stride stays the layer width's
    for n_probes in (1, 64, 65, 128):
        form, r, lds, _ = plan(16385, [100, 300, 16], n_probes)
        assert form == PINGPONG and lds == 2 * 64 * (304 + 4) * 4


def test_every_form_leaves_room_for_the_epilogue_tables():
    """A condition on the plan: per row, a single-image form keeps z and p (2 x 33 floats), the key table (n_probes) and the
    first-occurrence mask (2) side by side; the two-image form keeps keys and mask on the image z no longer needs."""
    R = 32 * fc.cus()
    ns = sorted({130, 4097, 16384, 16385} | {fc.rows(n, R) for _, _, n in fc.CASES})
    seen = set()
    for dims in fc.ARCHS:
        for n in ns:
            for n_probes in range(1, 129):
                form, rows, lds, _ = plan(n, dims, n_probes)
                S = fc.row_stride(form, rows, lds)
                need = n_probes + 2 if form == PINGPONG else 66 + n_probes + 2
                assert need <= S, (dims, n, n_probes, form, S)
                assert S % 8 == 4                                       # S / 4 odd: conflict-free 16-byte LDS reads
                assert S >= 4 + max(-(-w // 8) * 8 for w in dims[:-1])   # and a whole activation row fits
                seen.add(form)
    assert seen == fc.ALL_FORMS


def test_the_grid_selects_the_forms_it_names():
    """The (form, architecture, n) grid of the GPU tests, against the plan -- with the CU count of this machine (256 without a
    device, the MI355X's)."""
    R = 32 * fc.cus()
    for case in fc.CASES:
        form, dims, n = case
        for n_probes in (1, 10, 64, 65, 128):
            assert plan(fc.rows(n, R), dims, n_probes)[0] == form, fc.case_id(case)
    assert {form for form, _, _ in fc.CASES} == fc.ALL_FORMS


def test_refusals_are_those_of_the_launch():
    L = _capi.lib()

    def rc(n, dims, n_probes):
        return L.nlsh_encode_form(n, len(dims) - 1, _capi.int_array(dims), n_probes, None, None, None, None)
    assert rc(100, NARROW, 1) == _capi.OK and rc(0, NARROW, 1) == _capi.OK
    assert rc(100, NARROW, 0) == _capi.E_INVALID and rc(100, NARROW, 129) == _capi.E_INVALID
    assert b"n_probes" in L.nlsh_last_error()
    assert rc(-1, NARROW, 1) == _capi.E_INVALID
    assert rc(100, [128, 633, 16], 1) == _capi.E_UNSUPPORTED and rc(100, [1025, 64, 16], 1) == _capi.E_UNSUPPORTED
    assert rc(100, [128, 64, 33], 1) == _capi.E_UNSUPPORTED
    assert rc(100, [128, 0, 16], 1) == _capi.E_INVALID
    assert L.nlsh_encode_form(100, 0, _capi.int_array([128]), 1, None, None, None, None) == _capi.E_INVALID
