"""The argument contract of Terrain.viewshed, panorama, cast and sight_height, in full: exception class and whole message of
every entry of the four BAD_CALLS tables, and the ordered rule list each call hands to ``_validate.run``
(tests/golden/terrain_call_errors.json).  The args modules match fragments; this ledger pins every byte and the order, so the
boundary code can be reorganised without moving a check.  No GPU and no library needed.

Re-record after a deliberate change of a message, a rule or a BAD_CALLS table, from the repository root:
    python -m tests.test_terrain_call_errors --record"""
import json
import os
import sys

import pytest

from horayzon_amd import _lib
from horayzon_amd import _validate as V
from tests import test_cast_args as tc
from tests import test_panorama_args as tp
from tests import test_sight_height_args as ts
from tests import test_viewshed_args as tv

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_call_errors.json")
MODULES = {"viewshed": tv, "panorama": tp, "cast": tc, "sight_height": ts}

# one valid call per rule list: (name in the fixture, module, method, arguments)
VALID_CALLS = [
    ("viewshed", tv, "viewshed", lambda: ((tv._obs(),), dict(visible=tv._vis(), seen_count=tv._seen(), cells_seen=tv._cells()))),
    ("sight_height", ts, "sight_height",
     lambda: ((ts._obs(), ts._tab()), dict(height=ts._height(), lowest=ts._lowest(), cells_reached=ts._cells()))),
    ("panorama", tp, "panorama",
     lambda: ((tp._obs(), tp._azim(), tp._elev(), 100.0),
              dict(dist=tp._dist(), point=tp._point(), hits=tp._hits(), vec_north=tp._frame(1), vec_norm=tp._frame(2)))),
    ("cast_directions", tc, "cast",
     lambda: ((tc._org(), tc._dirs()), dict(max_dist=9.0, occluded=tc._occ(), dist=tc._dist(), point=tc._point()))),
    ("cast_targets", tc, "cast",
     lambda: ((tc._org(),), dict(targets=tc._tgt(), occluded=tc._occ(), dist=tc._dist(), point=tc._point()))),
]


def _forbidden():
    raise AssertionError("the library was called")


def bad_calls(method):
    """[class name, message] of every BAD_CALLS entry of the method's args module, in table order."""
    mod, seen = MODULES[method], []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "lib", _forbidden)
        for make, _, _ in mod.BAD_CALLS:
            args, kw = make()
            try:
                getattr(mod._terrain(), method)(*args, **kw)      # (a call that passes the checks ends at the library)
            except Exception as e:                                   # noqa: BLE001 -- the class is what is recorded
                seen.append([type(e).__name__, str(e)])
    return seen


def rule_order(mod, method, make):
    """[class name, message] of every rule one valid call hands to ``V.run``, in order.  The Terrain is not initialised, so
    the call ends at that guard (or at the forbidden library), after its rules."""
    seen, run = [], V.run

    def recording_run(rules):
        rules = list(rules)
        seen.extend([exc.__name__, message] for exc, message, _ in rules)
        run(rules)
    t = mod._terrain()
    t._shape = None
    args, kw = make()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "lib", _forbidden)
        mp.setattr(V, "run", recording_run)
        with pytest.raises((_lib.HorayzonHipError, AssertionError)):
            getattr(t, method)(*args, **kw)
    return seen


def collect():
    return {"bad_calls": {method: bad_calls(method) for method in MODULES},
            "rule_order": {name: rule_order(mod, method, make) for name, mod, method, make in VALID_CALLS}}


@pytest.fixture(scope="module")
def ledger():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("method", list(MODULES))
def test_every_bad_call_raises_the_recorded_class_and_message(ledger, method):
    recorded, now = ledger["bad_calls"][method], bad_calls(method)
    assert len(now) == len(recorded), "BAD_CALLS of %s changed: re-record the fixture" % method
    for i, (want, got) in enumerate(zip(recorded, now)):
        assert got == want, "%s, BAD_CALLS[%d]" % (method, i)


@pytest.mark.parametrize("name", [name for name, _, _, _ in VALID_CALLS])
def test_the_rules_are_the_recorded_ones_in_the_recorded_order(ledger, name):
    mod, method, make = next(v[1:] for v in VALID_CALLS if v[0] == name)
    now = rule_order(mod, method, make)
    assert now, "no rule reached _validate.run"
    assert now == ledger["rule_order"][name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_terrain_call_errors --record")
    with open(FIXTURE, "w") as f:
        json.dump(collect(), f, indent=1)
        f.write("\n")
