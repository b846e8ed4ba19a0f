"""The primitive-map shape sweep without a GPU: every guard of tests/pmap_shape_util.py (assertions on the inputs
and the oracle's outputs alone: each case reaches the branch of gcs_pmap.hip it is in the table for) and the
oracle on every case.  Run with -s to see what the tables reach."""
import numpy as np
import pytest

import pmap_shape_util as U
from oracle import primitive_map as opm


def test_select_table_reaches_every_branch():
    rep = U.select_table_guards()
    show = {k: sorted(v) if isinstance(v, set) else v for k, v in rep.items() if k != "hiword"}
    print("\nselect table:", len(U.SELECT_CASES), "cases")
    for k in ("paths", "kernels", "M", "k", "sh", "other", "dense_empty_minus_k", "leaves", "last_leaf", "k_eq_M"):
        print(f"  {k}: {show[k]}")
    print("  hiword_ties tiles (case, position, group, of it inside the first k):", len(rep["hiword"]))


def test_fuse_tables_reach_every_branch():
    rep = U.fuse_table_guards()
    print("\nfuse tables:")
    for cid, r in rep.items():
        print(f"  {cid}: {r}")


def test_key_restatement_orders_as_the_oracle():
    """ord_key / tile_keys (what the guards count with) give the oracle's order on every weight pattern."""
    rng = np.random.default_rng(5)
    for pattern in U.PATTERNS:
        for mode in ("view", "evict"):
            t = U.pattern_tile(rng, 1500, 900, pattern, 64, mode)
            keys, _ = U.tile_keys(t, mode)
            got = np.argsort(keys, kind="stable")[:200].astype(np.int32)
            ref = (opm.select_topk_slots(t["weights"], t["valid_mask"], 200) if mode == "view" else
                   opm.select_lowest_mass_slots(t["weights"], t["valid_mask"], t["last_supported_scan_seq"], U.SCAN_SEQ,
                                                opm.GC_RECENCY_DECAY_LAMBDA, 200))
            assert np.array_equal(got, ref), (pattern, mode)


@pytest.mark.parametrize("case", U.SELECT_CASES, ids=[c.id for c in U.SELECT_CASES])
def test_select_case_oracle(case):
    tiles, order, P = U.build_select_case(case)
    n = len(order)
    assert 4 <= n <= 6 and U.ABSENT_ID in order[1:-1]
    for pos, s in enumerate(case.tiles):
        if s is not None:
            assert int(tiles[U.tile_id(pos)]["valid_mask"].sum()) == s.n_valid   # exact valid counts
    if case.mode == "view":
        v = U.select_oracle(case, tiles, order, P)
        assert v["candidate_slots"].shape == (n * case.k,) and v["positions"].shape == (n * case.k, 3)
        assert np.isfinite(v["positions"]).all()
        for i in range(n):   # every tile's slots are distinct
            assert len(np.unique(v["candidate_slots"][i * case.k:(i + 1) * case.k])) == case.k
    else:
        assert len(np.unique(P["w"][0])) == case.k
        res, nxt = U.select_oracle(case, tiles, order, P)
        assert nxt == 1000 + n * case.k and sum(r[0] for r in res) == n * case.k > 0
        for tid in order:
            assert int(tiles[tid]["valid_mask"].sum()) >= case.k


@pytest.mark.parametrize("case", U.FUSE_CASES, ids=[c.id for c in U.FUSE_CASES])
def test_fuse_case_oracle(case):
    d = U.build_fuse_case(case.id)
    assert d["assoc"]["candidate_tile_ids"].shape == (case.N, case.K) and U.INACTIVE_ID not in d["active"]
    tiles, nxt, st = U.fuse_oracle(case.id)
    assert st["insert_count_total"] > 0 and st["fused_count"] > 0 and st["merged_count"] == 0
    assert nxt == U.NEXT_ID + st["insert_count_total"] and set(d["active"]) <= set(tiles)
    for t in tiles.values():
        assert t["weights"].shape == (U.M_FUSE,) and np.isfinite(t["Lambdas"]).all()
