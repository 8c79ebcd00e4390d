"""The host's choice of the decode GEMV prologue's form (mi355x_rows_prologue_plan: no launch,
no device access): lanes per superblock and passes over the row, by K and the workgroup's waves.
The widest form with nb * lanes <= 64 * waves takes the row in one pass on as many waves as the
workgroup has; rows that fill the workgroup keep 16 lanes per superblock and up to 3 passes."""
import pytest


@pytest.mark.parametrize("K,waves,lanes,passes", [
    (2048, 6, 32, 1),    # q/k/v, o-proj: 8 superblocks on 4 of 6 waves
    (2048, 12, 64, 1),   # gate + up, the head: 8 of 12 waves
    (5632, 12, 32, 1),   # down: 22 superblocks on 11 of 12 waves
    (4096, 6, 16, 1),    # fills 4 of 6 waves at 16 lanes, too long for 32
    (28672, 12, 16, 3),  # Llama-3-70B ffn_down: three passes of 48 superblocks
    (256, 6, 64, 1),
])
def test_pinned_forms(K, waves, lanes, passes):
    import ggml_mi355x as g
    assert g.rows_prologue_plan(K, waves) == (lanes, passes)


def test_rule():
    import ggml_mi355x as g
    for waves in range(1, 13):
        for nb in range(1, 145):
            got = g.rows_prologue_plan(256 * nb, waves)
            if nb > 12 * waves:  # more than 3 passes of 4 superblocks per wave
                assert got == g.E_UNSUPPORTED, (nb, waves, got)
                continue
            lanes, passes = got
            assert lanes in (16, 32, 64)
            want = 64 if nb * 64 <= 64 * waves else 32 if nb * 32 <= 64 * waves else 16
            assert lanes == want, (nb, waves, got)
            if lanes > 16:
                assert passes == 1 and nb * lanes <= 64 * waves
            else:
                assert passes == -(-nb // (4 * waves)) and 1 <= passes <= 3


def test_long_streams_keep_16_lanes():
    """A launch whose waves stream more than two 16-superblock steps keeps 16 lanes per
    superblock (measured slower with the wide forms); up to two steps the rule above holds."""
    import ggml_mi355x as g
    for K, waves, wide in ((2048, 6, 32), (2048, 12, 64), (4096, 12, 32), (5632, 12, 32)):
        for steps in (0, 1, 2):
            assert g.rows_prologue_plan(K, waves, steps) == (wide, 1)
        for steps in (3, 10, 1000):
            lanes, passes = g.rows_prologue_plan(K, waves, steps)
            assert lanes == 16 and passes == -(-(K // 256) // (4 * waves))


def test_arguments():
    import ggml_mi355x as g
    assert g.rows_prologue_plan(2048, 0) == g.E_INVAL
    assert g.rows_prologue_plan(2048, 6, -1) == g.E_INVAL
    assert g.rows_prologue_plan(2048, 13) == g.E_INVAL
    assert g.rows_prologue_plan(2000, 6) == g.E_INVAL
    assert g.rows_prologue_plan(0, 6) == g.E_INVAL
    assert g.rows_prologue_plan(256 * 145, 12) == g.E_UNSUPPORTED
