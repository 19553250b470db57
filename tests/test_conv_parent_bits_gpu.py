"""The forward sparse convolution, one case per dispatch route (cv_sp_conv_f32 / launch_rows / launch_finish), against
recorded bits: tests/golden/conv_parent_bits.json holds, for every case, the sha256 of the bytes of the whole
sentinel-padded output buffer as the library wrote it before the epilogues and the launch statements were folded into one
each.  Every case is also checked against the float64 oracle by the helper that runs it (tests/test_conv_paths_gpu.py).

The outputs are deterministic - partial tiles are summed in a fixed order, the ticket route included - and the refactor
moved no arithmetic, so the hashes are expected to be EQUAL.  The model axis has no case of its own:
tests/test_net_models_gpu.py demands torch.equal with the one-model runs that this table pins."""
import contextlib
import hashlib
import json
import os

import pytest

from canonicalvoting_amd import me as ME
from tests.test_conv_paths_gpu import (_clean_flag, _manager, _pinned_split_target,     # noqa: F401  (autouse fixtures)
                                       acc_in_halves, expected_splits, run_fwd, word_epilogue_fp32)

pytestmark = pytest.mark.gpu
BITS = os.path.join(os.path.dirname(__file__), "golden", "conv_parent_bits.json")
HL = dict(pieces=2, in_hl=True, out_hl=True, res_hl=True)


@contextlib.contextmanager
def option(name, value):
    prev = ME.set_option(name, value)
    try:
        yield
    finally:
        ME.set_option(name, prev)


def _wp(pieces, j_end):
    return lambda: run_fwd(300, "box", 5, 32, 64, pieces=pieces, flavour=1, j_range=(0, j_end))


def _hl_splits(n, splits):
    def run():
        assert expected_splits(n, 64, 27, 32) == splits
        return run_fwd(n, "box", 3, 32, 64, **HL)
    return run


def _groups(n, cout, groups, in_hl, zskip=None):
    def run():
        perms = _manager(n, "mixed").mask_perms(3, 1, groups)
        with option("zskip", zskip) if zskip is not None else contextlib.nullcontext():
            assert not zskip or (ME.option("zskip") and getattr(perms, "_cv_has_map", False)), "what makes the dispatcher set gvalid"
            return run_fwd(n, "mixed", 3, 32, cout, pieces=2 if in_hl else 3, in_hl=in_hl, out_hl=in_hl, row_perm=perms,
                           perm_groups=groups)
    return run


def _hd(shape):
    def run():
        assert ME.option("hd_mask") & 4 and ME.option("hd_min_rows") <= 16384, "the defaults that send 96 columns to conv_hd"
        with option("hd_shape", shape):
            return run_fwd(16384, "box", 3, 32, 96, pieces=2, in_hl=True, out_hl=True)
    return run


CASES = {
    "rows_f32": lambda: run_fwd(300, "mixed", 3, 40, 32, pieces=3),                 # conv_rows<1, false>, conv_finish
    "rows_scalar": lambda: run_fwd(129, "mixed", 3, 32, 30, pieces=3),              # word epilogue, conv_finish_scalar
    "rows_vec29": lambda: run_fwd(300, "box", 5, 32, 64, pieces=3, flavour=1, j_range=(0, 29)),     # conv_rows<2, true>
    "wp3_10": _wp(3, 10), "wp2_10": _wp(2, 10), "wp1_10": _wp(1, 10),               # conv_rows_wp<2, P, 10>, direct
    "wp3_28": _wp(3, 28), "wp2_28": _wp(2, 28), "wp1_28": _wp(1, 28),               # conv_rows_wp<2, P, 28>, direct
    "wp3_split": lambda: run_fwd(700, "mixed", 3, 64, 96, pieces=3),                # conv_rows_wp<3, 3> + conv_finish
    "hl_nb1": lambda: run_fwd(300, "mixed", 3, 32, 32, **HL),                       # conv_hl<1 / 3 / 2> + finish
    "hl_nb3": lambda: run_fwd(300, "mixed", 3, 32, 96, **HL),
    "hl_wide": lambda: run_fwd(300, "mixed", 3, 32, 256, **HL),
    "hl_small16": _hl_splits(6144, 16),                                             # conv_finish_small
    "hl_finish17": _hl_splits(5770, 17),                                            # conv_finish
    "hl_direct": lambda: run_fwd(700, "mixed", 1, 64, 64, **HL),                    # conv_hl, unsplit epilogue
    "hl_tickets": lambda: run_fwd(700, "mixed", 3, 32, 64, tickets=True, **HL),     # in-launch reduction
    "groups2_f32": _groups(700, 64, 2, False),                                      # mask groups, nbr_perm, gvalid
    "groups3_hl": _groups(3000, 96, 3, True),
    "groups3_hl_zskip": _groups(3000, 96, 3, True, zskip=1),
    "hd_shape0": _hd(0), "hd_shape1": _hd(1), "hd_shape2": _hd(2),                  # conv_hd<3,8,3> / <3,4,2> / <3,8,2>
    "hd_1x1": lambda: run_fwd(16384, "box", 1, 32, 96, pieces=2, in_hl=True, out_hl=True),
    "stem3": lambda: run_fwd(700, "box", 5, 3, 32, pieces=2, out_hl=True, stem=True),       # conv_stem_mfma
    "stem6": lambda: run_fwd(700, "box", 5, 6, 32, pieces=2, out_hl=True, stem=True),
    "acc_in_wide": lambda: acc_in_halves(2, 0),                                     # acc_in, float4 epilogue of conv_finish
    "acc_in_words": lambda: word_epilogue_fp32(3, 2),                               # acc_in, word epilogue of conv_finish
}


def buffer_hash(buf):
    return hashlib.sha256(buf.contiguous().cpu().numpy().tobytes()).hexdigest()


def _recorded():
    with open(BITS) as f:
        return json.load(f)


def test_every_case_has_recorded_bits():
    assert set(_recorded()) == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_recorded_bits(name):
    got = buffer_hash(CASES[name]())
    assert got == _recorded()[name], name + ": the output buffer is not the bits the parent wrote"
