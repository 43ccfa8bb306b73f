"""CPU-only: every workspace size query of the C ABI returns what tests/golden/workspace_bytes.json records for it (per query the values
of each argument and the results at their product, written by tools/workspace_table.py from the sources before the workspaces were
carved by one helper)."""
import itertools
import json
import os

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")


@pytest.fixture(scope="module")
def L():
    from fvgp_amd import _lib
    _lib.build()
    return _lib.lib()


def _records():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_every_size_query():
    from fvgp_amd import _lib
    queries = {s for s in _lib.SYMBOLS + _lib.SYMBOLS_NN if s.endswith("_bytes")}
    assert queries and queries == {r["symbol"] for r in _records()}


def test_every_result_still_holds(L):
    total, wrong = 0, []
    for r in _records():
        points = list(itertools.product(*r["axes"]))
        assert len(points) == len(r["results"])
        total += len(points)
        wrong += [(r["symbol"], a, want, got) for a, want in zip(points, r["results"]) for got in [int(getattr(L, r["symbol"])(*a))] if got != want]
    assert total > 1000
    assert not wrong, f"{len(wrong)} of {total} results moved, the first: {wrong[:5]}"
