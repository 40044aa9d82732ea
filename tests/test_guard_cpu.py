"""tests/_guard.py catches what it is for. Pure numpy: the download is a host array that a stand-in for the kernel has
written, correctly or with one defect; every defect must be reported with its position."""
import numpy as np
import pytest

from fmi_amd import DType
from tests import _guard as G
from tests import _fp8 as F
from tests import _half as H

N = 515 * 4 + 3  # f32: two whole 256-lane tiles, three lane groups, a 3-element tail


def want_f32(n=N):
    return (np.arange(n, dtype=np.float32) * np.float32(0.37) - np.float32(300.0)).astype(np.float32)


def launch(lay, poison, want, skip=(), stray=()):
    """The allocation after a kernel that stored `want` but for the element indices in `skip`, and that also stored the
    byte 0x01 at the body-relative byte offsets in `stray`."""
    raw = G.image(lay, poison)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(lay.n, -1).copy()
    body = raw[lay.body:lay.body + lay.nbytes].reshape(lay.n, -1)
    keep = np.ones(lay.n, bool)
    keep[list(skip)] = False
    body[keep] = w[keep]
    for off in stray:
        raw[lay.body + off] = 0x01
    return raw


@pytest.mark.parametrize("offset", [0, 1])
def test_a_correct_launch_passes_and_the_body_comes_back(offset):
    want, lay = want_f32(), G.Layout(N, np.float32, offset)
    (p,) = G.poisons_for(want, np.float32)
    got = G.check_image(launch(lay, p, want), lay, p, want, "correct")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert lay.body == G.FRONT + 4 * offset and lay.body % 16 == 4 * offset
    assert lay.total - lay.body - lay.nbytes >= 2 * 256 * 16 and G.FRONT == 4096


@pytest.mark.parametrize("skip,named", [((0,), "element 0 unwritten"), ((N - 1,), f"element {N - 1} unwritten"),
                                        (tuple(range(512 * 4, 512 * 4 + 4)), f"element {512 * 4} unwritten: 4 of")])
def test_unwritten_elements_are_reported_with_their_position(skip, named):
    """Index 0, index n - 1, one 16-B lane group."""
    want, lay = want_f32(), G.Layout(N, np.float32)
    (p,) = G.poisons_for(want, np.float32)
    with pytest.raises(AssertionError, match=named):
        G.check_image(launch(lay, p, want, skip=skip), lay, p, want, "case")


@pytest.mark.parametrize("stray,named", [((4 * N,), r"guard written.*first at body \+ %d \(output bytes \+ 0\)" % (4 * N)),
                                         ((-1,), r"guard written.*first at body - 1:"),
                                         (tuple(range(4 * N + 4096, 4 * N + 8192)),
                                          r"4096 guard byte\(s\) changed, first at body \+ %d \(output bytes \+ 4096\)" % (4 * N + 4096))])
@pytest.mark.parametrize("offset", [0, 1])
def test_stray_writes_are_reported_with_their_position(stray, named, offset):
    """One byte at body + nbytes, one at body - 1, one whole tile past the end (the second tile of the back guard)."""
    want, lay = want_f32(), G.Layout(N, np.float32, offset)
    (p,) = G.poisons_for(want, np.float32)
    with pytest.raises(AssertionError, match=named):
        G.check_image(launch(lay, p, want, stray=stray), lay, p, want, "case")
    with pytest.raises(AssertionError, match="guard written"):
        G.check_image(launch(lay, p, want, stray=stray), lay, p, None, "guards alone")


def test_a_guard_declared_one_element_early_reports_the_last_store():
    want, lay = want_f32(), G.Layout(N, np.float32)
    raw = launch(lay, G.GUARD_BYTE, want)
    assert not G.occurs(G.GUARD_BYTE, want, np.float32)
    with pytest.raises(AssertionError, match=r"guard written.*first at body \+ %d \(output bytes \+ 0\)" % (4 * (N - 1))):
        G.check_image(raw, lay.shortened(N - 1), G.GUARD_BYTE, want[:N - 1], "declared early")
    G.check_image(raw, lay, G.GUARD_BYTE, want, "declared right")


def test_a_modified_input_is_reported_with_its_position():
    x, lay = want_f32(), G.Layout(N, np.float32, 1)
    before = G.image(lay, x.view(np.uint8))
    G.check_frozen(before.copy(), before, lay, "intact")
    after = before.copy()
    after[lay.body + 4 * 7 + 2] ^= 0x10
    with pytest.raises(AssertionError, match=r"input modified.*first at body \+ 30 \(element 7\)"):
        G.check_frozen(after, before, lay, "in place on a peer")
    after = before.copy()
    after[lay.body + lay.nbytes] = 0
    with pytest.raises(AssertionError, match="guard written"):
        G.check_frozen(after, before, lay, "past an input")


# ---- the poison rule -----------------------------------------------------------------------------------------------------
def test_chooser_never_returns_a_pattern_that_is_in_want():
    rng = np.random.default_rng(5)
    for dtype in (np.uint8, np.uint16, np.float32, np.int64, np.float64):
        size = np.dtype(dtype).itemsize
        for trial in range(40):
            want = rng.integers(0, 256, 64 * size, dtype=np.uint8).view(dtype).copy()
            for c in G.CANDIDATES:  # random bytes but for the candidates' patterns ...
                want.view(G.UINT[size])[want.view(G.UINT[size]) == G.pattern(c, dtype)] = 0
            planted = G.CANDIDATES[:trial % (len(G.CANDIDATES))]  # ... then the first k candidates occur in want
            for k, c in enumerate(planted):
                want.view(G.UINT[size])[3 + 5 * k] = G.pattern(c, dtype)
            ps = G.poisons_for(want, dtype)
            assert len(ps) == 1 and ps[0] == G.CANDIDATES[len(planted)] and not G.occurs(ps[0], want, dtype), (dtype, trial)
    xs = [np.full(4, G.pattern(0xA5, np.float32), np.uint32).view(np.float32), want_f32(8)]  # a group of outputs
    assert G.poisons_for(xs, np.float32) == (0x5A,)


def test_chooser_falls_back_to_two_runs_and_the_pair_judges_every_element():
    """A uint8 `want` that holds all 256 values: every candidate occurs. Under the pair, an element left unwritten is
    reported by at least one of the two runs whatever it should have held, and a single run refuses such a `want`."""
    want = np.tile(np.arange(256, dtype=np.uint8), 5)[:1277]
    ps = G.poisons_for(want, np.uint8)
    assert len(ps) == 2 and ps[0] != ps[1]
    lay = G.Layout(want.size, np.uint8)
    for p in ps:
        G.check_image(launch(lay, p, want), lay, p, want, "correct", paired=True)
        with pytest.raises(AssertionError, match="poison rule broken"):
            G.check_image(launch(lay, p, want), lay, p, want, "single run")
    for i in (0, int(ps[0]), int(ps[1]), 256 + int(ps[0]), want.size - 1):  # want[i] is a poison itself at three of these
        caught = 0
        for p in ps:
            try:
                G.check_image(launch(lay, p, want, skip=(i,)), lay, p, want, "skipped", paired=True)
            except AssertionError as e:
                assert f"element {i} unwritten" in str(e)
                caught += 1
        assert caught == (1 if want[i] in ps else 2), i


def test_nan_is_judged_on_raw_bits():
    """A want[i] that is NaN: an unwritten element (the poison's bits) is no match, although a NaN-tolerant comparison
    would pass a NaN poison; a NaN of other bits in `want` is no occurrence of the poison, a NaN with the poison's own
    bits is."""
    nan_poison = 0xFF  # f32 0xFFFFFFFF: a NaN
    assert np.isnan(np.array([G.pattern(nan_poison, np.float32)], np.uint32).view(np.float32)[0])
    want = want_f32(64)
    want[9] = np.nan  # 0x7FC00000
    assert not G.occurs(nan_poison, want, np.float32) and G.poisons_for(want, np.float32, (nan_poison, 0xA5)) == (nan_poison,)
    lay = G.Layout(64, np.float32)
    G.check_image(launch(lay, nan_poison, want), lay, nan_poison, want, "correct")
    raw = launch(lay, nan_poison, want, skip=(9,))
    body = raw[lay.body:lay.body + lay.nbytes].view(np.float32)
    assert np.isnan(body[9]) and np.isnan(want[9])  # what a NaN-matches-NaN comparison sees: nothing
    with pytest.raises(AssertionError, match="element 9 unwritten"):
        G.check_image(raw, lay, nan_poison, want, "NaN under a NaN poison")
    want.view(np.uint32)[9] = 0xFFFFFFFF  # the poison's own bits
    assert G.occurs(nan_poison, want, np.float32) and G.poisons_for(want, np.float32, (nan_poison, 0xA5)) == (0xA5,)


def test_no_candidate_is_a_nan_in_any_float_type():
    """So a kernel's own NaN (whose bits the hardware chooses) can never be taken for the poison."""
    for c in G.CANDIDATES + (G.GUARD_BYTE,):
        b = bytes([c])
        assert not np.isnan(np.frombuffer(b * 4, np.float32)[0]) and not np.isnan(np.frombuffer(b * 8, np.float64)[0])
        bits16 = np.frombuffer(b * 2, np.uint16)
        assert not H.is_nan(bits16, "f16")[0] and not H.is_nan(bits16, "bf16")[0]
        assert not F.is_nan(np.frombuffer(b, np.uint8), "e4m3")[0] and not F.is_nan(np.frombuffer(b, np.uint8), "e5m2")[0]


def test_layouts_of_packed_and_one_byte_types():
    lay = G.Layout(77, DType.F4E2M1)
    assert lay.nbytes == 39 and G.element_bytes(DType.F4E2M1) == 1
    with pytest.raises(ValueError):
        G.Layout(77, DType.F4E2M1, offset=1)
    assert G.Layout(77, DType.F4E2M1, offset=2).body == G.FRONT + 1
    lay = G.Layout(8255, DType.F8E4M3, 1)
    assert lay.nbytes == 8255 and lay.body == G.FRONT + 1
    assert G.Layout(5, DType.BF16, 1).body == G.FRONT + 2 and G.pattern(0xA5, DType.BF16) == 0xA5A5
