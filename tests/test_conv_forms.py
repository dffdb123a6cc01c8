"""CPU: train_engine.ConvForms, the lazy per-conv weight record of the training step.  Plain Python values
stand in for the packed weights; no GPU, no kernel."""
import pytest

from weatherconverter_amd.diffusion_model.models.train_engine import ConvForms


def _counting(calls, name, fn):
    def build(c):
        calls.append(name)
        return fn(c)
    return build


def test_builder_runs_once_on_first_read_not_at_construction():
    calls = []
    c = ConvForms(w=_counting(calls, 'w', lambda c: [1, 2, 3]))
    assert calls == []
    first = c.w
    assert first == [1, 2, 3] and calls == ['w']
    assert c.w is first and c.w is first and calls == ['w']


def test_has_runs_no_builder():
    calls = []
    c = ConvForms(w=_counting(calls, 'w', lambda c: 1), wn=_counting(calls, 'wn', lambda c: 2), f3h=None)
    assert c.has('w') and c.has('wn')  # lazy, not built
    assert not c.has('f3h') and not c.has('x6')  # given as None / not given
    assert calls == []
    assert c.wn == 2 and c.has('wn') and calls == ['wn']
    with pytest.raises(AttributeError, match='f3h'):
        c.f3h
    with pytest.raises(AssertionError):
        c.has('wm')  # a mistyped form name is an error, not "absent"
    with pytest.raises(AssertionError):
        ConvForms(wm=lambda c: 0)


def test_form_assigned_ahead_of_time_is_kept_and_never_built():
    calls = []
    c = ConvForms(wn=_counting(calls, 'wn', lambda c: 'built'))
    batch = object()
    c.wn = batch
    assert c.has('wn') and c.wn is batch and c.wn is batch and calls == []
    d = ConvForms()
    d.f3 = batch  # a form without a builder can be assigned too
    assert d.has('f3') and d.f3 is batch


def test_shared_relayout_is_built_once_and_only_if_needed():
    calls = []
    c = ConvForms(w=_counting(calls, 'w', lambda c: 10), x6=_counting(calls, 'x6', lambda c: c.w + 1),
                  f3h=_counting(calls, 'f3h', lambda c: c.w + 2), wn=_counting(calls, 'wn', lambda c: 99))
    assert c.wn == 99 and calls == ['wn']  # a form that does not read w leaves it unbuilt
    assert c.f3h == 12 and c.x6 == 11
    assert calls == ['wn', 'f3h', 'w', 'x6']
    assert c.w == 10 and calls.count('w') == 1
