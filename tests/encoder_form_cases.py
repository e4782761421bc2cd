"""The (form, architecture, n) grid of the encoder-form tests (tests/test_encoder_forms_cpu.py pins the plan on it,
tests/test_gpu_encoder_forms.py runs it).  Architectures are [d, hidden..., H]; a row count is an int or an expression in R = 32 * CUs
(one full round of 32-row workgroups), the CU count being the one `nlsh_encode_form` reports.  Nothing here touches the library at
import time."""
from nlsh_amd import _capi

H16, SINGLE, SINGLE_WIDE, BUILD128, PINGPONG, HET = (_capi.ENC_FORM_H16, _capi.ENC_FORM_SINGLE, _capi.ENC_FORM_SINGLE_WIDE,
                                                     _capi.ENC_FORM_BUILD128, _capi.ENC_FORM_PINGPONG, _capi.ENC_FORM_HET)
ALL_FORMS = {H16, SINGLE, SINGLE_WIDE, BUILD128, PINGPONG, HET}
LDS_LIMIT = 160 * 1024 - 256      # dynamic LDS a workgroup may ask for (ENC_LDS_LIMIT of csrc/encode_hash.hip)

# (form, row counts, architectures)
GRID = (
    (H16, (4095, 4096), ([50, 64, 64, 12], [128, 33, 1])),
    (SINGLE, (4097, 4129), ([25, 96, 8], [128, 33, 1], [1024, 64, 7], [960, 256, 256, 32], [40, 96, 128, 64, 32, 20])),
    (SINGLE, ("2*R+R//2+1",), ([320, 64, 8],)),
    (HET, ("R+1", "R+R//2"), ([25, 96, 8], [1024, 64, 7], [200, 256, 256, 24])),
    (HET, ("2*R+1",), ([320, 64, 8],)),
    (SINGLE_WIDE, (130, 4097), ([64, 257, 8], [128, 600, 16], [64, 632, 632, 32], [96, 320, 40, 32])),
    (SINGLE_WIDE, (16385,), ([32, 320, 8],)),
    (BUILD128, (16385, 16511), ([25, 96, 8], [312, 256, 16], [50, 64, 64, 12], [40, 96, 128, 64, 32, 20], [128, 33, 1])),
    (PINGPONG, (16385, 16447), ([100, 300, 16], [64, 260, 312, 24], [312, 257, 8])),
)
CASES = [(form, dims, n) for form, ns, archs in GRID for dims in archs for n in ns]      # [(form, dims, row-count spec)]
ARCHS = []
for _case in CASES:
    if _case[1] not in ARCHS:
        ARCHS.append(_case[1])


def cus():
    """CU count the plan's HET rule uses on this machine (256 without a device)."""
    return _capi.encode_form(1, [8, 8, 8])[3]


def rows(n, R):
    """A row-count spec of the grid for a round of R rows."""
    return eval(n, {"R": R}) if isinstance(n, str) else n


def case_id(case):
    form, dims, n = case
    return f"{_capi.ENC_FORM_NAMES[form]}-{'x'.join(map(str, dims))}-n{str(n).replace('//', 'd')}"


def max_rows(dims, R):
    """Most rows the grid runs an architecture at."""
    return max(rows(n, R) for _, d, n in CASES if d == dims)


def row_stride(form, rows_per_workgroup, lds_bytes):
    """S, the floats per row of a workgroup's LDS image, from the plan's LDS size (PINGPONG holds two images)."""
    images = 2 if form == PINGPONG else 1
    assert lds_bytes % (images * rows_per_workgroup * 4) == 0
    return lds_bytes // (images * rows_per_workgroup * 4)
