"""tests/sorted_build_checker.py without a GPU: the oracle's own lattice, renumbered and with its points permuted the way a right build
would leave it, passes; and each kind of fault a build could make is rejected BY NAME when injected alone -- notes/sorted_build_tests.md.
The checker is what tests/test_sorted_build.py holds the device's tables against, so a fault it let through would be a hole there."""
import numpy as np
import pytest

import sorted_build_checker as sc


@pytest.fixture(scope="module")
def lattice(po):
    """1001 points (three phantom points), d = 3: 300 identical points far from the origin (a long row per remainder), the rest spread
    over a few cells, none at the origin -- so the phantom points make vertices with empty rows."""
    rng = np.random.default_rng(11)
    N, d = 1001, 3
    f = (rng.random((N, d), np.float32) * 3.0 + 1.0).astype(np.float32)
    f[rng.permutation(N)[:300]] = np.float32([2.25, 1.5, 3.125])
    o = po.OracleCRF(N, 2)
    o.set_unary(np.zeros((N, 2), np.float32))
    o.add_pairwise(f, 1.0)
    ref = sc.reference_tables(o, 0)
    o.close()
    assert ref["offset"].shape[0] == 1004 and np.bincount(ref["offset"][:N].ravel(), minlength=ref["V"]).max() >= 300
    assert np.bincount(ref["offset"][:N].ravel(), minlength=ref["V"]).min() == 0          # the origin's vertices: empty rows
    return ref


@pytest.fixture()
def right(lattice):
    rng = np.random.default_rng(5)
    return sc.tables_from_reference(lattice, sc.row_major_order(lattice), rng.permutation(lattice["N"]))


def test_a_right_table_passes_under_any_renumbering_and_point_order(lattice, right):
    rng = np.random.default_rng(6)
    phi = sc.check(lattice, right, sorted_build=True)
    assert np.array_equal(phi, sc.row_major_order(lattice))
    # any numbering will do for the hash build; the sorted build's must be row-major
    anyhow = sc.tables_from_reference(lattice, rng.permutation(lattice["V"]), rng.permutation(lattice["N"]))
    sc.check(lattice, anyhow, sorted_build=False)
    with pytest.raises(sc.TableFault) as e:
        sc.check(lattice, anyhow, sorted_build=True)
    assert e.value.kind in ("fastn", "row-major ids")
    anyhow["fastn"] = None
    with pytest.raises(sc.TableFault) as e:
        sc.check(lattice, anyhow, sorted_build=True)
    assert e.value.kind == "row-major ids"
    # the identity: the reference's own numbering and order
    sc.check(lattice, sc.tables_from_reference(lattice, np.arange(lattice["V"]), np.arange(lattice["N"])), sorted_build=False)


def _long_row(t):
    v = int(np.argmax(np.diff(t["rowptr"])))
    return v, int(t["rowptr"][v]), int(t["rowptr"][v + 1])


def swap_in_long_row(t, ref):
    v, s, e = _long_row(t)
    assert e - s >= 300
    a, b = s + 100, s + 200
    for n in ("csr_pt", "csr_w"):
        t[n][[a, b]] = t[n][[b, a]]


def redirect_neighbour(t, ref):
    j = 1
    v = int(np.flatnonzero(t["nbr"][j, :, 1] >= 0)[3])
    t["nbr"][j, v, 1] = (t["nbr"][j, v, 1] + 1) % t["V"]


def exchange_sides(t, ref):
    j = 2
    v = int(np.flatnonzero((t["nbr"][j, :, 0] >= 0) & (t["nbr"][j, :, 1] >= 0))[0])
    t["nbr"][j, v] = t["nbr"][j, v, ::-1].copy()


def phantom_in_row(t, ref):
    v, s, e = _long_row(t)
    t["csr_pt"][e - 1] = ref["N"] + 1                      # (the last of the row: a phantom's original id is the largest, the order stays right)


def rowptr_off_by_one(t, ref):
    v, s, e = _long_row(t)
    t["rowptr"][v + 1] -= 1


def fastn_bit(t, ref):
    t["fastn"][7] ^= 1


def merge_ids(t, ref):
    a = int(t["offset"][0, 0])
    b = int(t["offset"][np.flatnonzero((t["offset"] != a).all(1))[0], 0])
    t["offset"][t["offset"] == b] = a


def bary_bit(t, ref):
    t["bary"].view(np.int32)[17, 1] ^= 1


def stale_weight(t, ref):
    t["csr_w"].view(np.int32)[5] ^= 1


def entry_twice(t, ref):
    v = int(np.flatnonzero(np.diff(t["rowptr"]) == 2)[0])
    s = int(t["rowptr"][v])
    t["csr_pt"][s + 1] = t["csr_pt"][s]


FAULTS = [
    ("two entries of a long row swapped", swap_in_long_row, "row order"),
    ("one neighbour redirected", redirect_neighbour, "neighbour redirected"),
    ("n1 / n2 exchanged on one axis", exchange_sides, "neighbours exchanged"),
    ("a phantom listed in a row", phantom_in_row, "phantom in a row"),
    ("rowptr off by one", rowptr_off_by_one, "rowptr"),
    ("one fastn bit wrong", fastn_bit, "fastn"),
    ("two ids merged", merge_ids, "renumbering"),
    ("one bit of a barycentric weight", bary_bit, "bary"),
    ("one bit of a row's weight", stale_weight, "row weight"),
    ("an entry listed twice", entry_twice, "row content"),
]


@pytest.mark.parametrize("name,inject,kind", FAULTS, ids=[f[0].replace(" ", "_") for f in FAULTS])
def test_every_fault_is_rejected_by_name(lattice, right, name, inject, kind):
    sc.check(lattice, right, sorted_build=True)
    inject(right, lattice)
    with pytest.raises(sc.TableFault) as e:
        sc.check(lattice, right, sorted_build=True)
    assert e.value.kind == kind, (name, str(e.value))
    assert sc.KINDS[kind] in str(e.value)


def test_a_point_order_that_moves_a_phantom_is_rejected(lattice, right):
    right["perm"][[0, -1]] = right["perm"][[-1, 0]]
    with pytest.raises(sc.TableFault) as e:
        sc.check(lattice, right, sorted_build=True)
    assert e.value.kind == "perm"
