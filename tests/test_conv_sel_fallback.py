"""CPU test of train_graph._conv(sel=...): y2_conv_fwd_sel is asked after the algorithm was chosen; where it refuses (Y2_ENOSUP, nothing launched) the plain
y2_conv_fwd runs and the caller is told; any other code is an error.  Against a stand-in library object: no GPU, no launch."""
import ctypes

import pytest
import torch

import _hip
from model import train_graph as tg


class StandIn(object):
    """Records the calls; y2_conv_fwd_sel answers `sel_rc`."""

    def __init__(self, sel_rc):
        self.sel_rc, self.calls = sel_rc, []

    def y2_conv_fwd_sel(self, p, gamma, z_sel, ldzs, st):
        q = ctypes.cast(p, ctypes.POINTER(_hip.ConvParams)).contents
        self.calls.append(('sel', q.algo, q.tile, gamma.value, z_sel.value, ldzs))
        return self.sel_rc

    def y2_conv_fwd(self, p, st):
        q = ctypes.cast(p, ctypes.POINTER(_hip.ConvParams)).contents
        self.calls.append(('plain', q.algo, q.tile))
        return 0


def run(monkeypatch, sel_rc, sel=True):
    chosen = []

    def choose(p, dev, **kw):
        chosen.append(kw)
        p.algo, p.tile = _hip.ALGO_WINOGRAD_IMPLICIT, 3

    monkeypatch.setattr(_hip, 'autotune_conv', choose)
    monkeypatch.setattr(_hip, 'conv_workspace', lambda p, dev: None)
    L = StandIn(sel_rc)
    B, H, W, cin, cout = 2, 8, 8, 32, 64
    x, u, z = torch.zeros(B, H, W, cin), torch.zeros(16 * cout * cin), torch.zeros(B, H, W, cout)
    gamma, z_sel = torch.ones(cout), torch.zeros(B, H // 2, W // 2, cout)
    out = tg._conv(L, None, x, None, z, B, H, W, cin, cin, cout, 3, cout, u=u, u_eligible=True, sel=(gamma, z_sel) if sel else None)
    assert len(chosen) == 1 and 'sel' not in chosen[0]          # the choice is the plain problem's: same table key
    return L.calls, out, gamma, z_sel


def test_served_by_the_sel_entry(monkeypatch):
    calls, out, gamma, z_sel = run(monkeypatch, 0)
    assert calls == [('sel', _hip.ALGO_WINOGRAD_IMPLICIT, 3, gamma.data_ptr(), z_sel.data_ptr(), 64)]
    assert out == (None, True)


def test_refusal_falls_back_to_the_plain_entry(monkeypatch):
    calls, out, _, _ = run(monkeypatch, _hip.ENOSUP)
    assert [c[0] for c in calls] == ['sel', 'plain'] and calls[1] == ('plain', _hip.ALGO_WINOGRAD_IMPLICIT, 3)
    assert out == (None, False)


def test_any_other_code_is_an_error(monkeypatch):
    with pytest.raises(RuntimeError, match='y2_conv_fwd_sel'):
        run(monkeypatch, -1)


def test_without_sel_nothing_changes(monkeypatch):
    calls, out, _, _ = run(monkeypatch, 0, sel=False)
    assert [c[0] for c in calls] == ['plain'] and out is None
    assert _hip.ENOSUP == -3 and 'Y2_ENOSUP' in _hip.ERRORS[_hip.ENOSUP]
