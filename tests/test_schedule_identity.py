"""Bit identity of the launch schedule (tulip.jl_amd/csrc/schedule.cpp: build_schedule) across changes that do not mean to alter it.

The schedule -- every task list and launch list a handle replays for its whole life -- is built on the host, deterministically, and an analysis-only handle
(Backend(device=-1)) exports nearly all of it.  For every (case, configuration) below ONE SHA-256 is taken over, in a fixed order,
  * every name tlpk_symbolic_get serves on such a handle (NAMES: all of them but chain_trace, krylov_unsolved, chain_retries and row_block), each as the
    bytes of its int64 array, behind its name and length;
  * the tlpk_info fields the schedule writes (INFO): flops as hex floats, counts as ints.  Timing fields are left out.  (flops_update_skipped is not a
    field of tlpk_info and so is not covered.)
and compared FOR EQUALITY with tests/golden/schedule_digests.json.  There is no tolerance.  Beside each digest the fixture keeps the lengths of the main
task lists and the sorted set of launch kinds, so that a mismatch says where to look.  (The file is compact: one line per configuration with one
"<sha256>/<shape>" per case, "=" where the record is the default configuration's, and one line per distinct shape = lengths + kinds; _pack / _unpack.)

The fixture is re-recorded only by a change that MEANS to alter the schedule, or by a compiler change; it names the `hipcc --version` and the commit it
was recorded with.  A change that must keep the schedule (a refactoring) records it from a build of its PARENT commit -- a copy of the parent tree with
this one file (and the export names it reads) added, the same hipcc -- and never from the code under test:

    python tests/test_schedule_identity.py --record tests/golden/schedule_digests.json PARENT_HASH

--record refuses to write a fixture in which some configuration's digests equal the default's on every case, or in which a launch kind that
build_schedule can emit (the LaunchKind enum of tlpk_host.hpp, less the ones marked unused) never occurs.

Four knobs (TLPK_DEFER_UPPER, TLPK_SKIP_WIN, TLPK_EA_BANDS, TLPK_UPD_LPT) are fixed by the first analysis of a process, so every configuration runs in a
fresh child process (CPU only): one child per configuration analyses all the cases.

Cases: the smallest ones that reach each branch.
  golden instances   tiny LPs: one or two small fronts
  r420x700           fronts wider than 64 and 256 columns, no chain
  gs1400             general sparse LP, one dense front: chain, split-K of every launch
  gs1400-splitk0     the same without split-K by tile count (a case setting, as TLPK_STREAMS below): launches this small are otherwise always cut by
                     position, and the K-length split (TLPK_KSPLIT_LEN) never acts
  gs2600             the same with a top front of f >= 2048 rows: the TLPK_EA_BANDS branch, front assembly under TLPK_FA_MIN_F
  gs2700-macro       eleven block columns in macro columns narrower than the front (TLPK_MACRO_TILES=200) and a chain: the tiles TLPK_CHAIN_JIT holds back
  ba8, ba8-streams1, ba8-rank0of2, ba8-rank1of2, ba8-k2
                     block-angular, 8 blocks of three block columns + linking rows: two stream groups, upper fronts, root front, LK_WAIT_UPPER, side fork /
                     join; one stream group; the two ranks of a sharded job; the augmented system
  ba8-merge0         the same with TLPK_SOLVE_MERGE=0: levels this small otherwise always merge their small fronts into the sweep, and TLPK_SOLVE_SIDE never acts
  ba17               17 blocks: more multi-block-column fronts on a level than the look-ahead rule (16) and the chain rule (8) take
  skip2x1600         the LP and settings of tests/test_symbolic.py's skip-list test (TLPK_SKIP_MIN_F=64, TLPK_SPLITK_TILES=0): update tiles with skip
                     lists (upd_seg), which TLPK_SKIP_WIN and TLPK_UPD_LPT act on
  ba4                the LP of tests/test_symbolic.py's tail-shape test (launches that fill TLPK_TAIL64_SLOTS = 4 slots)
  dense_cols         dense columns as augmented nodes
  stair25            many small and single fronts, thin triangular solves, the small-front merge"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import functools
import hashlib
import json
import re
import subprocess

import numpy as np
import pytest

import tulip_jl_amd as tk
from helpers import block_angular, load_golden, random_lp_matrix

FIXTURE = os.path.join(HERE, "golden", "schedule_digests.json")
ROOT = os.path.dirname(HERE)

FRONT_FIELDS = ["front_eatab", "front_f", "front_lda", "front_ns", "front_col0", "front_parent", "front_loff", "front_rowoff", "front_reloff", "front_child_ptr",
                "front_nchild", "front_flagoff", "front_ucoff", "front_uoff", "front_ubuf"]
NAMES = ["perm", "etree", "colcount", "s_colptr", "s_rowidx", "s_target", "s_diag_row", "pair_ptr", "pair_j", "rowidx", "rel", "ea_tab", "children", "depth",
         "front_block", "front_group", "ngroups", "front_local", "col_local", "row_local", "root_front", "dense_cols", *FRONT_FIELDS,
         "potrf_tasks", "trsm_tasks", "update_tasks", "upd_seg", "trsm_early", "update_tile64", "skip_off", "skip_bits", "front_single", "reduce_tasks",
         "chain_items", "chain_counters", "fa_tasks", "front_fa", "front_upper", "ea_tasks",
         "fwd_gather_tasks", "fwd_diag_tasks", "fwd_update_tasks", "bwd_update_tasks", "fwd_small_tasks", "bwd_small_tasks", "fwd_sweep_tasks", "bwd_sweep_tasks",
         "n_sweep_flags", "gth_ptr", "gth_src", "factor_launches", "fwd_launches", "bwd_launches",
         "launch_meta", "zero_tasks", "zero_small", "singles"]
INFO = ["flops_update", "flops_update_chain", "flops_update_alg_chain", "launches_update", "launches_solve", "chain_launches", "chain_items"]
LENGTHS = ["update_tasks", "reduce_tasks", "chain_items", "upd_seg", "ea_tasks", "fa_tasks"]

# configuration -> environment (one knob at a time, but for the knobs that only act together)
CONFIGS = {
    "default": {},
    "chain0": {"TLPK_CHAIN": "0"},
    "chain1": {"TLPK_CHAIN": "1"},
    "chain_jit1": {"TLPK_CHAIN_JIT": "1"},
    "chain_early0": {"TLPK_CHAIN_EARLY": "0"},
    "chain_tile64_0": {"TLPK_CHAIN_TILE64": "0"},
    "chain_tile64_1": {"TLPK_CHAIN_TILE64": "1"},
    "lookahead0": {"TLPK_LOOKAHEAD": "0"},
    "lookahead1": {"TLPK_LOOKAHEAD": "1"},
    "la_full1": {"TLPK_LA_FULL": "1"},
    "la_macro0": {"TLPK_LA_MACRO": "0"},
    "macro_tiles50": {"TLPK_MACRO_TILES": "50", "TLPK_LOOKAHEAD": "0"},
    "ksplit_len512": {"TLPK_KSPLIT_LEN": "512"},
    "splitk_tiles0": {"TLPK_SPLITK_TILES": "0"},
    "tail_slots16": {"TLPK_TAIL_SLOTS": "16"},
    "tail64": {"TLPK_TAIL64": "3", "TLPK_TAIL64_SLOTS": "4", "TLPK_SPLITK_TILES": "0", "TLPK_CHAIN": "0"},      # the values of tests/test_symbolic.py
    "upd_lpt1": {"TLPK_UPD_LPT": "1"},
    "upd_super2": {"TLPK_UPD_SUPER": "2"},
    "skip_win256": {"TLPK_SKIP_WIN": "256"},
    "ea_bands2": {"TLPK_EA_BANDS": "2"},
    "defer_upper0": {"TLPK_DEFER_UPPER": "0"},
    "sweep0": {"TLPK_SWEEP": "0"},
    "solve_merge0": {"TLPK_SOLVE_MERGE": "0"},
    "solve_side1": {"TLPK_SOLVE_SIDE": "1"},
    "solve_one_group0": {"TLPK_SOLVE_ONE_GROUP": "0"},
    "potrf_mode2": {"TLPK_POTRF_MODE": "2"},
    "fa_min_f512": {"TLPK_FA_MIN_F": "512", "TLPK_FA_DENSITY": "0"},          # (knobs of the analysis, not of the schedule: they switch the front-assembly lists on)
}
# a configuration whose digests must differ from ANOTHER one's too: the tail shape from the settings it rides on
ALSO_DIFFERS = {"tail64": {"TLPK_SPLITK_TILES": "0", "TLPK_CHAIN": "0"}}


@functools.lru_cache(maxsize=None)
def _ba(nblocks):
    """diagonal blocks whose top fronts have ~590 pivot columns: three block columns each"""
    return block_angular(nblocks=nblocks, mk=700, nk=1400, m0=100, nnz_in=4, link_prob=0.5, seed=3)


def _ba_case(nblocks, system="K1", env=None, **kw):
    A, rb = _ba(nblocks)
    return A, system, dict(row_block=rb, **kw), env or {}


def _general(m):
    sys.path.insert(0, ROOT)
    from workloads import general_sparse_lp
    return general_sparse_lp(m)


def _skip_case():
    sys.path.insert(0, ROOT)
    from workloads import block_angular_lp
    A, rb = block_angular_lp(nblocks=2, mk=1600, nk=3200, m0=150)
    return A, "K1", dict(row_block=rb), {"TLPK_SKIP_MIN_F": "64", "TLPK_SPLITK_TILES": "0"}


def _stair25():
    from tulip_jl_amd.problem import read_free_mps, standard_form
    return standard_form(read_free_mps(os.path.join(HERE, "golden", "stair25.mps"))).A


def _dense_cols():
    from test_dense_cols import planted
    return planted(300, 700, 3, [60 + (7 * t) % 90 for t in range(40)], 70)[0]


# case -> () -> (A, "K1" | "K2", Backend arguments, environment of the case)
CASES = {f"golden-{g['name']}": (lambda g=g: (g["A_csc"], "K1", {}, {})) for g in load_golden()}
CASES.update({
    "r420x700": lambda: (random_lp_matrix(420, 700, 6, 11), "K1", {}, {}),
    "gs1400": lambda: (_general(1400), "K1", {}, {}),
    "gs1400-splitk0": lambda: (_general(1400), "K1", {}, {"TLPK_SPLITK_TILES": "0"}),
    "gs2600": lambda: (_general(2600), "K1", {}, {}),
    "gs2700-macro": lambda: (_general(2700), "K1", {}, {"TLPK_MACRO_TILES": "200", "TLPK_CHAIN_MIN_NS": "257"}),
    "ba8": lambda: _ba_case(8),
    "ba8-streams1": lambda: _ba_case(8, env={"TLPK_STREAMS": "1"}),
    "ba8-rank0of2": lambda: _ba_case(8, rank=0, nranks=2),
    "ba8-rank1of2": lambda: _ba_case(8, rank=1, nranks=2),
    "ba8-k2": lambda: _ba_case(8, system="K2"),
    "ba8-merge0": lambda: _ba_case(8, env={"TLPK_SOLVE_MERGE": "0"}),
    "ba17": lambda: _ba_case(17),
    "skip2x1600": lambda: _skip_case(),
    "ba4":lambda: (lambda A, rb: (A, "K1", dict(row_block=rb), {}))(*block_angular(nblocks=4, mk=300, nk=600, m0=200, nnz_in=3, link_prob=0.9, seed=5)),
    "dense_cols": lambda: (_dense_cols(), "K1", dict(dense_cols="auto", dense_col_min=40, relax=1), {}),
    "stair25": lambda: (_stair25(), "K1", {}, {}),
})


def schedule_record(case):
    """one analysis on the host -> the record the fixture stores.  The caller has set the configuration's environment."""
    A, system, kw, env = CASES[case]()
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        kkt = tk.setup(A, tk.K1() if system == "K1" else tk.K2(), tk.Backend(device=-1, **kw))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    h = hashlib.sha256()
    arrays = {}
    for name in NAMES:
        a = np.ascontiguousarray(kkt.symbolic(name), dtype=np.int64)
        arrays[name] = a
        h.update(f"{name}:{a.size};".encode()); h.update(a.tobytes())
    st = kkt.stats()
    for key in INFO:
        v = st[key]
        h.update(f"{key}={float(v).hex() if isinstance(v, float) else int(v)};".encode())
    kinds = sorted({int(k) for name in ("factor_launches", "fwd_launches", "bwd_launches") for k in arrays[name].reshape(-1, 3)[:, 0]})
    kkt.close()
    return {"sha256": h.hexdigest(), "len": {name: int(arrays[name].size) for name in LENGTHS}, "kinds": kinds}


def config_records(config):
    """the records of every case under one configuration, from a fresh child process"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("TLPK_")}
    env.update(CONFIGS[config] if isinstance(config, str) else config)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.splitlines()[-1])


def emitted_kinds():
    """LaunchKind enum of tlpk_host.hpp -> {name: value} of the kinds build_schedule can emit (all but the ones the header marks unused)"""
    src = open(os.path.join(ROOT, "tulip.jl_amd", "csrc", "tlpk_host.hpp")).read()
    body = src[src.index("enum LaunchKind"):]
    body = body[body.index("{") + 1:body.index("};")]
    unused = set(re.findall(r"(LK_\w+)\s*/\*\s*unused", body))
    body = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", body), flags=re.S)
    names = [t.split("=")[0].strip() for t in body.split(",") if t.strip()]
    assert names[0] == "LK_EXTEND_ADD" and all(n.startswith("LK_") for n in names)
    return {n: v for v, n in enumerate(names) if n not in unused}


def _pack(records):
    """records[config][case] -> the fixture's compact rows: per configuration one "<sha256>/<shape>" per case in the order of CASES ("=": the record of
    the default configuration), and the distinct shapes [lengths in the order of LENGTHS, launch kinds]"""
    shapes = []

    def one(rec):
        shape = [[rec["len"][name] for name in LENGTHS], rec["kinds"]]
        if shape not in shapes:
            shapes.append(shape)
        return f"{rec['sha256']}/{shapes.index(shape)}"
    rows = {config: ["=" if config != "default" and per_case[c] == records["default"][c] else one(per_case[c]) for c in CASES]
            for config, per_case in records.items()}
    return rows, shapes


def _unpack(fx):
    assert fx["cases"] == list(CASES) and fx["lengths"] == LENGTHS

    def one(s):
        sha, shape = s.split("/")
        lens, kinds = fx["shapes"][int(shape)]
        return {"sha256": sha, "len": dict(zip(LENGTHS, lens)), "kinds": kinds}
    default = [one(s) for s in fx["records"]["default"]]
    return {config: {c: default[j] if s == "=" else one(s) for j, (c, s) in enumerate(zip(fx["cases"], row))} for config, row in fx["records"].items()}


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    return {"hipcc_version": fx["hipcc_version"], "parent_commit": fx["parent_commit"], "records": _unpack(fx)}


def fixture_faults(records):
    """the conditions --record insists on; [] = none violated"""
    faults = []
    for config in CONFIGS:
        others = ["default"] if config != "default" else []
        for other in others:
            if all(records[config][c]["sha256"] == records[other][c]["sha256"] for c in CASES):
                faults.append(f"configuration {config}: every digest equals that of {other}")
    for config, base in ALSO_DIFFERS.items():
        if all(records[config][c]["sha256"] == records["base:" + config][c]["sha256"] for c in CASES):
            faults.append(f"configuration {config}: every digest equals that of {base}")
    seen = {k for per_case in records.values() for rec in per_case.values() for k in rec["kinds"]}
    faults += [f"launch kind {n} = {v} never occurs" for n, v in emitted_kinds().items() if v not in seen]
    return faults


def test_fixture_covers_every_case_names_its_origin_and_meets_its_conditions():
    fx = recorded()
    assert "version" in fx["hipcc_version"].lower() and re.fullmatch(r"[0-9a-f]{40}", fx["parent_commit"])
    assert sorted(fx["records"]) == sorted(list(CONFIGS) + ["base:" + c for c in ALSO_DIFFERS])
    for config, per_case in fx["records"].items():
        assert sorted(per_case) == sorted(CASES), config
        for rec in per_case.values():
            assert sorted(rec) == ["kinds", "len", "sha256"] and sorted(rec["len"]) == sorted(LENGTHS)
    assert fixture_faults(fx["records"]) == []
    assert emitted_kinds()["LK_CHAIN"] == 22 and len(emitted_kinds()) == 23


def _compare(got, want, config):
    bad = {}
    for case in CASES:
        print(f"{config} {case}: {got[case]}")
        if got[case] != want[case]:
            bad[case] = {"got": got[case], "recorded": want[case]}
    assert not bad, f"schedule differs from the one recorded at {recorded()['parent_commit'][:12]}: {json.dumps(bad, indent=1)}"


@pytest.mark.parametrize("config", list(CONFIGS))
def test_schedule_equals_the_recorded_one(config):
    _compare(config_records(config), recorded()["records"][config], config)


def _record(path, parent):
    ver = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    out = {"hipcc_version": " | ".join(s.strip() for s in ver[:2]), "parent_commit": parent, "records": {}}
    for config in CONFIGS:
        out["records"][config] = config_records(config)
        print(config, json.dumps({c: r["sha256"][:12] for c, r in out["records"][config].items()}), flush=True)
    for config, base in ALSO_DIFFERS.items():
        out["records"]["base:" + config] = config_records(base)
    faults = fixture_faults(out["records"])
    if faults:
        raise SystemExit("NOT written:\n  " + "\n  ".join(faults))
    rows, shapes = _pack(out["records"])
    with open(path, "w") as f:           # (one line per configuration and per shape: the file stays small enough to read)
        f.write("{\n" + "".join(f' {json.dumps(k)}: {json.dumps(v)},\n' for k, v in
                                [("hipcc_version", out["hipcc_version"]), ("parent_commit", parent), ("cases", list(CASES)), ("lengths", LENGTHS)]))
        f.write(' "records": {\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in rows.items()) + "\n },\n")
        f.write(' "shapes": [\n' + ",\n".join(f"  {json.dumps(v)}" for v in shapes) + "\n ]\n}\n")


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        print(json.dumps({case: schedule_record(case) for case in CASES}))
    elif len(sys.argv) == 4 and sys.argv[1] == "--record" and re.fullmatch(r"[0-9a-f]{40}", sys.argv[3]):
        _record(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit("usage: python tests/test_schedule_identity.py --record PATH PARENT_COMMIT_HASH")
