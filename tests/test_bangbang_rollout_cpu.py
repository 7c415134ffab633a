"""The inputs of tests/test_bangbang_rollout_gpu.py exercise the controllers: under the oracle, at
every shape of its window-against-loop test with more than one house, both bang-bang controllers
switch houses on and off, have "on" requests refused by the lockout, and (deadband form) hold
houses inside the band.  Keeps the GPU shapes from degenerating silently (e.g. a deadband so wide
that no house is ever switched back on inside the test's ticks)."""
import random

import numpy as np
import pytest

import golden_util as gu
from bangbang_inputs import CTRLS, SEED, SHAPES, overrides
from oracle import env_np as O


def oracle_events(n, ticks, ctrl):
    """The ticks of the GPU test's first rollout under the oracle and the controller: off->on
    switches, on->off switches, 'on' requests of a locked-out house, and decisions the deadband
    form takes from the current state inside the band."""
    props = gu.props_from_overrides(overrides(n))
    ora = O.OracleEnv(props, random.Random(SEED))
    db = props.cluster_prop.house_prop.deadband
    tg = ora.pop["target"]
    ups = downs = refused = holds = 0
    for _ in range(ticks):
        on0 = ora.on.copy()
        if ctrl == "bangbang":
            a = O.bangbang(ora.T, tg)
        else:
            a = O.deadband_bangbang(ora.T, tg, db, ora.on)
            holds += int(np.sum((ora.T >= tg - db / 2) & (ora.T <= tg + db / 2)))
        o, _ = ora.step(a)
        on1 = np.asarray(o["on"], bool)
        ups += int(np.sum(~on0 & on1))
        downs += int(np.sum(on0 & ~on1))
        refused += int(np.sum(np.asarray(a, bool) & ~on0 & ~on1))
    return ups, downs, refused, holds


@pytest.mark.parametrize("ctrl", CTRLS)
@pytest.mark.parametrize("n,ticks,win", [s for s in SHAPES if s[0] >= 2])
def test_shapes_exercise_the_controllers(n, ticks, win, ctrl):
    ups, downs, refused, holds = oracle_events(n, ticks, ctrl)
    print(f"n={n} ticks={ticks} {ctrl}: ups={ups} downs={downs} refused={refused} holds={holds}")
    assert ups > 0 and downs > 0 and refused > 0
    if ctrl == "deadband_bangbang":
        assert holds > 0
