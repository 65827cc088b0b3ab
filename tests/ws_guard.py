"""Guarded workspaces for the tests of the C ABI.

Every composite entry works inside memory the caller sizes with a `*_bytes` function.  `guarded(nbytes, fill, device)`
returns a handle whose `.view` is a uint8 view of EXACTLY `nbytes`, pre-filled with the byte `fill`, between a front guard
and a back guard of GUARD bytes each inside one allocation.  The guards hold a fixed, position-dependent byte pattern;
`.intact()` says whether a call wrote into one.  GUARD is 4 KiB (the tail tests/test_posterior_layers_gpu.py uses), a
multiple of every alignment the library asks for, so the view is aligned as the allocation is.

FILLS is the standard pair of hostile contents: 0x00, and 0xFF, which reads as NaN in fp32 and bf16, as -1 in any integer
and as a full counter in a ticket word.

Every handle is registered; the autouse fixture `ws_guards` (import it by name into a test module) asserts after each test
that every handle made during it is intact, then clears the registry.

Guards sit in front of and behind a workspace: they cannot see one region of a layout running into the next.  The
unequal-width and oracle tests remain the check for that."""
import pytest
import torch

GUARD = 4096
FILLS = (0x00, 0xFF)
_REGISTRY = []


def _pattern(n, device):
    """The guard bytes: 0xA5 xor a ramp of period 251, so that neither a constant fill nor a shifted copy matches."""
    return (torch.arange(n, dtype=torch.int64, device=device) % 251).to(torch.uint8) ^ 0xA5


class Guarded:
    def __init__(self, nbytes, fill, device, what=""):
        nbytes = int(nbytes)
        assert nbytes >= 0, nbytes
        assert 0 <= int(fill) <= 0xFF, fill
        self.nbytes, self.fill, self.what = nbytes, int(fill), what
        self.whole = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        self._want = _pattern(GUARD, self.whole.device)
        self.whole[:GUARD] = self._want
        self.whole[GUARD + nbytes:] = self._want
        self.view = self.whole[GUARD:GUARD + nbytes]
        self.view.fill_(self.fill)

    def refill(self, fill):
        """Overwrite the view (not the guards) with the byte `fill`."""
        self.fill = int(fill)
        self.view.fill_(self.fill)
        return self

    def numel(self):
        return self.nbytes

    def data_ptr(self):
        """The view's address (torch reports 0 for an empty view; this is where it would start)."""
        return self.whole.data_ptr() + GUARD

    def intact(self):
        """None when both guards are whole, else (side, first damaged offset inside that guard, damaged bytes in it) of the
        first damaged guard, "front" before "back"."""
        for side, got in (("front", self.whole[:GUARD]), ("back", self.whole[GUARD + self.nbytes:])):
            bad = got != self._want
            if bool(bad.any()):
                return side, int(torch.nonzero(bad)[0, 0]), int(bad.sum())
        return None

    def check(self):
        bad = self.intact()
        assert bad is None, (f"workspace {self.what!r} of {self.nbytes} declared bytes: {bad[2]} byte(s) of the {bad[0]} guard "
                             f"written, the first at guard offset {bad[1]}")


def guarded(nbytes, fill, device="cuda", what=""):
    h = Guarded(nbytes, fill, device, what)
    _REGISTRY.append(h)
    return h


def check_all():
    """Assert every registered handle intact and clear the registry (cleared even when one is damaged)."""
    handles = list(_REGISTRY)
    del _REGISTRY[:]
    for h in handles:
        if h.whole.is_cuda:
            torch.cuda.synchronize(h.whole.device)
            break
    for h in handles:
        h.check()


@pytest.fixture(autouse=True)
def ws_guards():
    del _REGISTRY[:]
    yield
    check_all()
