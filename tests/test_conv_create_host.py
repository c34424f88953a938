"""CPU: rsk_conv_create_host (include/rsk_codec.h), the host twin of rsk_conv_create_batch, against
tests/conv_create_ref: the reference's recorded SConn per packet out of one resolve -> create, the index that
survives the next batch, random equivalence with the host procedure, full tables, u_max and repeated calls,
skew, poisoned columns, optional outputs, the argument checks and determinism.  tests/test_gpu_conv_create.py
runs the same scenarios on the device."""
from __future__ import annotations

import pytest

from rsock_amd import codec as rc
from tests import conv_create_ref as C
from tests import conv_ref as R


@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_reference_pin_server(name):
    C.scenario_golden_server(rc, name, "cpu")


@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_survives_the_next_batch(name):
    C.scenario_survives(rc, name, "cpu")


@pytest.mark.parametrize("capacity", C.CAPACITIES)
@pytest.mark.parametrize("n", C.SIZES)
def test_random_equivalence(n, capacity):
    C.scenario_random(rc, n, capacity, True, True, "cpu")


@pytest.mark.parametrize("by_dst,by_id", R.FLAG_COMBOS)
@pytest.mark.parametrize("n,capacity", C.FLAG_POINTS)
def test_flag_combinations(n, capacity, by_dst, by_id):
    C.scenario_random(rc, n, capacity, by_dst, by_id, "cpu")


@pytest.mark.parametrize("kind", ["fewer", "none", "cap1_vacant", "cap1_live"])
def test_table_full(kind):
    C.scenario_full(rc, kind, "cpu")


@pytest.mark.parametrize("u_max", [1, 64, 65])
def test_u_max_repeated_calls(u_max):
    C.scenario_u_max(rc, u_max, "cpu")


def test_u_max_until_full():
    C.scenario_u_max_full(rc, "cpu")


@pytest.mark.parametrize("kind", ["one_key", "all_keys"])
def test_skew(kind):
    C.scenario_skew(rc, kind, "cpu")


BAND_TABLES = {}


@pytest.mark.parametrize("pattern", R.BAND_PATTERNS)
@pytest.mark.parametrize("n", R.BAND_SIZES)
def test_counts_on_colliding_rows(n, pattern):
    """The convs born in the call take rows that share one run of the device's LDS row table (tests/collide.py)."""
    assert C.scenario_band_create(rc, n, pattern, "cpu", cache=BAND_TABLES) > 600


def test_reads():
    C.scenario_reads(rc, "cpu")


def test_optional_outputs():
    C.scenario_optional_outputs(rc, "cpu")


def test_argument_errors():
    C.check_einval(rc, "cpu")


def test_determinism():
    C.scenario_determinism(rc, "cpu")
