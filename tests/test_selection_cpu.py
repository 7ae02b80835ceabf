"""The host-side algorithm selection (_hip.autotune_conv / wgrad_choice / conv_wgrad) decides what tests/golden/selection.json says it decides: table
keys, known / pinned / static choices, what a measurement would time and in which order, what is applied to the params.  No GPU: selection_cases.py."""
import copy
import json
import os

import pytest

from conftest import ROOT

import _hip
import selection_cases


@pytest.fixture(scope='module')
def golden():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'selection.json')))


@pytest.fixture(scope='module')
def dumped():
    if not os.path.exists(_hip.LIB_PATH):
        _hip.build()
    before = {k: getattr(_hip, k) for k in list(selection_cases.BASE) + ['_TUNE']}
    d = selection_cases.dump(_hip)
    assert all(getattr(_hip, k) is v for k, v in before.items())          # the dump leaves the module's switches as it found them
    return d


def test_selection_equals_the_recorded_one(golden, dumped):
    assert len(golden['keys']) >= 250 and sum(len(rs) for rs in golden['cases'].values()) >= 1500
    diff = selection_cases.differences(golden, dumped)
    assert not diff, '%d records differ from tests/golden/selection.json (from %s):\n%s' % (len(diff), golden['source'], '\n'.join(diff[:20]))


def test_the_grid_reaches_every_rule(golden):
    """The fixture is only worth what it covers: every algorithm, every special tile, a missing operand, both capturing answers and every
    y2_wino_wgrad_ex form appear in it."""
    cases = golden['cases']
    chosen = {tuple(r[2]) for case in ('table.peek', 'static', 'force.fused3', 'force.implicit3', 'force.split', 'force.split.f16', 'grad.f43') for r in cases[case] if isinstance(r[2], list)}
    assert {a for a, _ in chosen} == {0, 1, 2, 3, 4, 5, 6}
    timed = {tuple(c) for case in cases if case.startswith('candidates') for r in cases[case] for c in r[2]}
    assert {a for a, _ in timed} == {0, 1, 2, 3, 4, 5, 6} and {t for a, t in timed if a == 0} == {5, 3, 2, 1, 6, 8, 9, 15, 13, 12, 11}
    assert any(r[2] == 'OperandMissing' for r in cases['table.apply.pruned']) and any(r[2] == 'OperandMissing' for r in cases['static.pruned'])
    assert any(r[2] is None for r in cases['persist.off.peek']) and all(r[2] == [0, 13] for r in cases['persist.on.peek'])
    assert {r[2][-1] for r in cases['wgrad.capturing']} == {'y2_conv_wgrad', 'y2_wino_wgrad'}
    launched = {n for case in cases if case.startswith('wgrad.given') for r in cases[case] for n in r[2]}
    assert {'y2_wino_wgrad_ex:%d' % m for m in (1, 2, 3, 6, 7)} <= launched and {'scratch_ex:%d' % m for m in (0, 1, 2, 3, 6)} <= launched
    assert {r[3] for r in cases['wgrad.timed.v1']} == {0, 1} and {r[3] for r in cases['wgrad.timed.v0']} == {1}          # the forward-cost correction of the large maps


def test_a_changed_record_is_reported(golden):
    changed = copy.deepcopy(golden)
    record = changed['cases']['static'][5]
    record[2] = [record[2][0], record[2][1] + 1]
    diff = selection_cases.differences(golden, changed)
    assert len(diff) == 1 and diff[0].startswith('static %s:' % golden['problems'][record[0]])
    rekeyed = copy.deepcopy(golden)
    rekeyed['keys'][3] = rekeyed['keys'][3][:-1] + [not rekeyed['keys'][3][-1]]          # one element of one key: every record that asked it
    assert len(selection_cases.differences(golden, rekeyed)) == sum(r[1] == 3 for rs in golden['cases'].values() for r in rs) >= 1
    short = copy.deepcopy(golden)
    del short['cases']['candidates'][-1]
    del short['cases']['timed.ties']
    assert len(selection_cases.differences(golden, short)) == 2
