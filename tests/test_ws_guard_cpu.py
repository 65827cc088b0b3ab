"""CPU: tests/ws_guard.py itself, on CPU tensors - a damaged guard is reported with its side, offset and size, a write
inside the view is not, the view keeps the allocation's alignment, and the autouse fixture fails a test that leaves a
damaged handle behind."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import ws_guard
from ws_guard import FILLS, GUARD, guarded, ws_guards  # noqa: F401  (the fixture is used by name)

HERE = os.path.dirname(os.path.abspath(__file__))


def test_constants():
    assert FILLS == (0x00, 0xFF)
    assert GUARD == 4096
    nan32 = torch.full((4,), 0xFF, dtype=torch.uint8).view(torch.float32)
    nan16 = torch.full((2,), 0xFF, dtype=torch.uint8).view(torch.bfloat16)
    assert bool(torch.isnan(nan32).all()) and bool(torch.isnan(nan16).all())
    assert int(torch.full((8,), 0xFF, dtype=torch.uint8).view(torch.int64)[0]) == -1


@pytest.mark.parametrize("nbytes", [0, 1, 17, 4096, 100003])
@pytest.mark.parametrize("fill", FILLS)
def test_view_is_exact_filled_and_between_guards(nbytes, fill):
    h = guarded(nbytes, fill, "cpu")
    assert h.view.dtype == torch.uint8 and h.view.numel() == nbytes
    assert h.whole.numel() == nbytes + 2 * GUARD                      # a zero-byte request still yields guards
    assert h.data_ptr() == h.whole.data_ptr() + GUARD
    assert nbytes == 0 or h.view.data_ptr() == h.data_ptr()           # torch gives an empty view the address 0
    assert bool((h.view == fill).all())
    assert h.intact() is None
    # the guards hold a pattern, not a constant: neither fill reproduces it
    for g in (h.whole[:GUARD], h.whole[GUARD + nbytes:]):
        assert len(torch.unique(g)) > 100
        assert not bool((g == fill).all())


@pytest.mark.parametrize("nbytes", [0, 1, 4096, 100003])
def test_alignment_is_the_allocations(nbytes):
    h = guarded(nbytes, 0xFF, "cpu")
    for a in (16, 64, 256, 4096):
        assert h.data_ptr() % a == h.whole.data_ptr() % a
        assert nbytes == 0 or h.view.data_ptr() % a == h.whole.data_ptr() % a


@pytest.mark.parametrize("nbytes", [0, 24, 5000])
@pytest.mark.parametrize("side,off", [("front", 0), ("front", GUARD - 1), ("back", 0), ("back", GUARD - 1)])
def test_one_damaged_byte_is_reported_with_side_and_offset(nbytes, side, off):
    h = guarded(nbytes, 0x00, "cpu")
    pos = off if side == "front" else GUARD + nbytes + off
    h.whole[pos] ^= 0x01
    assert h.intact() == (side, off, 1)
    with pytest.raises(AssertionError, match=f"{side} guard"):
        h.check()
    h.whole[pos] ^= 0x01                                              # repaired: the fixture finds it whole
    assert h.intact() is None


def test_count_and_first_offset_of_a_damaged_run():
    h = guarded(64, 0xFF, "cpu")
    h.whole[GUARD + 64 + 10:GUARD + 64 + 30] = 0                      # an overrun of 20 bytes, 10 behind the end
    side, first, count = h.intact()
    assert side == "back" and first == 10 and 19 <= count <= 20       # a pattern byte may equal 0 by chance: at most one
    h.whole[0] ^= 0xFF                                                # the front guard is reported first
    assert h.intact() == ("front", 0, 1)
    ws_guard._REGISTRY.remove(h)


@pytest.mark.parametrize("fill", FILLS)
def test_writes_inside_the_view_are_not_reported(fill):
    h = guarded(333, fill, "cpu")
    h.view[0] = 0x5A
    h.view[-1] = 0x5A                                                 # the view's last byte
    h.view.view(-1)[1:-1] = 0x11
    assert h.intact() is None
    h.refill(fill ^ 0xFF)
    assert bool((h.view == (fill ^ 0xFF)).all()) and h.intact() is None


def test_registry_holds_the_tests_handles_and_check_all_clears_it():
    assert ws_guard._REGISTRY == []                                   # the fixture starts every test empty
    a, b = guarded(8, 0, "cpu"), guarded(0, 0xFF, "cpu")
    assert ws_guard._REGISTRY == [a, b]
    ws_guard.check_all()
    assert ws_guard._REGISTRY == []
    c = guarded(8, 0, "cpu", what="c")
    c.whole[GUARD + 8] ^= 0x80                                        # the first byte behind the view
    with pytest.raises(AssertionError, match="'c' of 8 declared bytes.*back guard.*offset 0"):
        ws_guard.check_all()
    assert ws_guard._REGISTRY == []                                   # cleared even when a handle was damaged


_INNER = """
import torch
from ws_guard import GUARD, guarded, ws_guards


def test_clean():
    h = guarded(32, 0xFF, "cpu")
    h.view[-1] = 1


def test_overrun():
    h = guarded(32, 0xFF, "cpu")
    h.whole[GUARD + 32] ^= 0xFF


def test_underrun():
    h = guarded(32, 0x00, "cpu")
    h.whole[GUARD - 1] ^= 0xFF


def test_clean_after_the_damaged_ones():
    guarded(0, 0x00, "cpu")
"""


def test_fixture_fails_a_test_that_leaves_a_damaged_handle(tmp_path):
    """The fixture is what the GPU tests rely on, so it is run for real: a small module in a pytest of its own."""
    mod = tmp_path / "test_inner_guard.py"
    mod.write_text(textwrap.dedent(_INNER))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([HERE] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "--rootdir", str(tmp_path), "-rA",
                        str(mod)], capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    out = r.stdout + r.stderr
    assert r.returncode == 1, out
    assert "4 passed, 2 errors" in out, out                           # the bodies pass; the fixture's teardown is the error
    assert "PASSED test_inner_guard.py::test_clean\n" in out, out
    assert "ERROR test_inner_guard.py::test_overrun" in out and "ERROR test_inner_guard.py::test_underrun" in out, out
    assert "back guard" in out and "front guard" in out, out
