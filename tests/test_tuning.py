"""The decode launch's A/B and test hooks (csrc/fls_tuning.hpp): one typed
struct, DecodeTuning, filled once per decode call by read_decode_tuning().

1. tests/fuzz/tuning_dump.cpp prints every field for the environment it runs
   in; built with g++ -fsanitize=address,undefined and run under each hook's
   edge values, every field must equal the hook's documented parse (the table
   below: default, clamp, and the special cases written out).  The `list` part
   (l.*) keys a resident table's cached descriptor list: a launch hook must
   not change it, a list hook must.
2. No other file of csrc/ calls getenv on one of these names (the experiment
   library's own launcher apart).
CPU only (no GPU, no HIP)."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "duckdb-fastlane_amd" / "csrc"
BIG = 2**31 - 1   # "at least N": no upper bound but int's
K_FSST_DEFAULT = 8 | 4 | 64   # kFsstDefault (fls_decode.hpp)

# hook -> (field, default, min, max): present => clamp(atoi(text), min, max)
LIST_INTS = {
    "FLS_STATIC_PCT": ("l.static_pct", 100, 0, 100),
    "FLS_TAIL_PIECES": ("l.tail_pieces", 2, 1, 255),
    "FLS_BLOCKS_PER_CU": ("l.blocks_per_cu", 0, 0, 127),
    "FLS_GUIDED_MIN_VECS": ("l.guided_min_vecs", 0, 0, 64),
    "FLS_GUIDED_FACTOR": ("l.guided_factor", 2, 1, 255),
    "FLS_DICT_WG": ("l.dict_wg", 1, 0, 2),
    "FLS_DICT_WG_MIN_VECS_PER_CU": ("l.dict_wg_min_vecs_per_cu", 64, 0, 255),
    "FLS_DICT_WG_STREAMS": ("l.dict_wg_streams", 4, 1, 31),
}
LAUNCH_INTS = {
    "FLS_OVERLAP_CU_SPLIT": ("x.overlap_cu_split", 0, 0, 31),
    "FLS_OVERLAP_DECODE_BPC": ("x.overlap_decode_bpc", 1, 1, BIG),
    "FLS_OVERLAP_FSST_WPC": ("x.overlap_fsst_wpc", 12, 0, BIG),
    "FLS_OVERLAP_MIN_VECS_PER_CU": ("x.overlap_min_vecs_per_cu", 800, 0, BIG),
    "FLS_OVERLAP_DECODE_PRIO": ("x.overlap_decode_prio", 0, 0, 3),
    "FLS_FUSED_FSST16": ("x.fused_fsst16", 6, 0, 16),   # (6: FusedLaunch's; by launch size unless given)
    "FLS_FUSED_PIECE": ("x.fused_piece", 2, 1, 64),
    "FLS_FUSED_WPC": ("x.fused_wpc", 0, 0, BIG),
    "FLS_FUSED_STATIC_PCT": ("x.fused_static_pct", 0, 0, 100),
    "FLS_FUSED_TAIL": ("x.fused_tail", 0, 0, BIG),
    "FLS_FUSED_TAIL_SPLIT": ("x.fused_tail_split", 1, 1, 64),
    "FLS_FUSED_X": ("x.fused_x", 0, -BIG - 1, BIG),
    "FLS_FUSED_MIN_VECS_PER_CU": ("x.fused_min_vecs_per_cu", 0, 0, BIG),
    "FLS_FSST_VARIANT": ("x.fsst_variant", K_FSST_DEFAULT, -BIG - 1, BIG),
    "FLS_FSST_SEG_CAP": ("x.fsst_seg_cap", 4096, -BIG - 1, BIG),
    "FLS_FSST_WPC": ("x.fsst_wpc", 0, 0, BIG),
    "FLS_FSST_PIECE": ("x.fsst_piece", 0, 1, 64),   # (0: computed)
}
# hook -> (field, default): present => atoi(text) != 0
LAUNCH_BOOLS = {
    "FLS_OVERLAP_GUIDED": ("x.overlap_guided", 0),
    "FLS_FUSED_STATIC_FIRST": ("x.fused_static_first", 1),
    "FLS_FUSED_HALVING": ("x.fused_halving", 0),
}
INTS = {**LIST_INTS, **LAUNCH_INTS}
LIST_HOOKS = list(LIST_INTS) + ["FLS_DECODE_POLICY", "FLS_FSST_SEG"]
LAUNCH_HOOKS = list(LAUNCH_INTS) + list(LAUNCH_BOOLS) + ["FLS_FUSED"]
POLICY_FSST_NOSEG = 8


def atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def clamp(v, lo, hi):
    return min(hi, max(lo, v))


def strict(s):   # a whole number in 0..INT_MAX (fsst_config_check's FLS_ERR_CONFIG otherwise)
    return int(re.fullmatch(r"\s*[+-]?\d+", s) is not None and 0 <= int(s) <= BIG)


def expected(env):
    """Every line tuning_dump prints under env, from the tables above."""
    e = {}
    for name, (field, default, lo, hi) in INTS.items():
        e[field] = str(clamp(atoi(env[name]), lo, hi) if name in env else default)
    for name, (field, default) in LAUNCH_BOOLS.items():
        e[field] = str(int(atoi(env[name]) != 0) if name in env else default)
    seg = int(atoi(env["FLS_FSST_SEG"]) != 0) if "FLS_FSST_SEG" in env else 1
    e["x.fsst_seg"] = str(seg)
    flags = atoi(env["FLS_DECODE_POLICY"]) & 0xFF if "FLS_DECODE_POLICY" in env else 0
    e["l.flags"] = str(flags | (0 if seg else POLICY_FSST_NOSEG))
    if "FLS_FUSED" in env:
        v = atoi(env["FLS_FUSED"])
        e["x.fused"] = str(2 if v == 1 else clamp(v, 0, 2))
    else:
        e["x.fused"] = "1"
    e["x.fused_fsst16_given"] = str(int("FLS_FUSED_FSST16" in env))
    for name, field in (("FLS_FUSED_X", "x.fused_x_hook"), ("FLS_FSST_VARIANT", "x.fsst_variant_hook")):
        e[field + ".given"] = str(int(name in env))
        e[field + ".ok"] = str(strict(env[name]) if name in env else 1)
        e[field + ".text"] = env.get(name, "")
    e["blocks_per_cu_cap"] = str(max(1, atoi(env["FLS_BLOCKS_PER_CU"])) if "FLS_BLOCKS_PER_CU" in env else 0)
    e["list_is_default"] = str(int(all(e[f] == str(d) for f, d, _, _ in LIST_INTS.values()) and e["l.flags"] == "0"))
    return e


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = tmp_path_factory.mktemp("tuning") / "tuning_dump"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I", str(CSRC), str(ROOT / "tests" / "fuzz" / "tuning_dump.cpp"),
                    "-o", str(out)], check=True)
    base = {k: v for k, v in os.environ.items() if not k.startswith("FLS_")}

    def run(envs):   # one process: the environments one after the other, as between two decode calls
        args = [",".join(f"{k}={v}" for k, v in env.items()) for env in envs]
        r = subprocess.run([str(out)] + args, env=base, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, f"{envs}: sanitizer report\n{r.stderr[-4000:]}"
        parts = r.stdout.split("--\n")[:-1]
        assert len(parts) == len(envs)
        return [dict(line.split("=", 1) for line in p.splitlines()) for p in parts]
    return lambda env: run(env) if isinstance(env, list) else run([env])[0]


def list_part(d):
    return {k: v for k, v in d.items() if k.startswith("l.")}


def check(dump, env):
    """Every field under env (or each of a list of them) as the tables say"""
    envs = env if isinstance(env, list) else [env]
    gots = dump(envs)
    for e, got in zip(envs, gots):
        assert got == expected(e), e
    return gots if isinstance(env, list) else gots[0]


def test_defaults(dump):
    got = check(dump, {})
    # the defaults, written out
    assert list_part(got) == {"l.flags": "0", "l.static_pct": "100", "l.tail_pieces": "2", "l.blocks_per_cu": "0",
                              "l.guided_min_vecs": "0", "l.guided_factor": "2", "l.dict_wg": "1",
                              "l.dict_wg_min_vecs_per_cu": "64", "l.dict_wg_streams": "4"}
    assert got["x.fsst_seg"] == "1" and got["x.fused"] == "1" and got["x.fused_fsst16_given"] == "0"
    assert got["x.overlap_fsst_wpc"] == "12" and got["x.overlap_min_vecs_per_cu"] == "800"
    assert got["x.fsst_variant"] == str(K_FSST_DEFAULT) and got["x.fsst_seg_cap"] == "4096"
    assert got["blocks_per_cu_cap"] == "0" and got["list_is_default"] == "1"


def edge_values(lo, hi):
    if hi == BIG:   # below the minimum, the minimum, large values (no maximum but int's)
        return [lo - 1, lo, 1000000, BIG] if lo > -BIG - 1 else [-5, 0, 7, 123456]
    return [lo - 1, lo, hi, hi + 1]


@pytest.mark.parametrize("name", list(INTS))
def test_int_hook_edges(dump, name):
    field, default, lo, hi = INTS[name]
    vals = edge_values(lo, hi)
    for v, got in zip(vals, check(dump, [{name: str(v)} for v in vals])):
        assert got[field] == str(clamp(v, lo, hi)), (name, v)
    for got in check(dump, [{name: ""}, {name: "abc"}]):   # present: atoi gives 0
        assert got[field] == str(clamp(0, lo, hi)), name


@pytest.mark.parametrize("name", list(LAUNCH_BOOLS) + ["FLS_FSST_SEG"])
def test_bool_hook_values(dump, name):
    field = "x.fsst_seg" if name == "FLS_FSST_SEG" else LAUNCH_BOOLS[name][0]
    for text, want in (("-1", "1"), ("0", "0"), ("1", "1"), ("2", "1"), ("", "0"), ("abc", "0")):
        assert check(dump, {name: text})[field] == want, (name, text)


def test_decode_policy_is_a_flag_byte(dump):
    for text, want in (("-1", "255"), ("0", "0"), ("255", "255"), ("256", "0"), ("321", "65"), ("", "0"), ("abc", "0")):
        assert check(dump, {"FLS_DECODE_POLICY": text})["l.flags"] == want, text


def test_fused_modes(dump):
    for text, want in (("0", "0"), ("1", "2"), ("2", "2"), ("7", "2"), ("-1", "0"), ("", "0"), ("abc", "0")):
        assert check(dump, {"FLS_FUSED": text})["x.fused"] == want, text


def test_fsst_seg_sets_the_flag_and_the_descriptor_choice(dump):
    got = check(dump, {"FLS_FSST_SEG": "0"})
    assert got["l.flags"] == str(POLICY_FSST_NOSEG) and got["x.fsst_seg"] == "0"
    got = check(dump, {"FLS_FSST_SEG": "1"})
    assert got["l.flags"] == "0" and got["x.fsst_seg"] == "1"
    got = check(dump, {"FLS_FSST_SEG": "0", "FLS_DECODE_POLICY": "64"})
    assert got["l.flags"] == str(64 | POLICY_FSST_NOSEG)


def test_blocks_per_cu_key_and_cap(dump):
    for text, key, cap in (("0", "0", "1"), ("1", "1", "1"), ("3", "3", "3"), ("127", "127", "127"),
                           ("200", "127", "200"), ("-4", "0", "1"), ("", "0", "1")):
        got = check(dump, {"FLS_BLOCKS_PER_CU": text})
        assert (got["l.blocks_per_cu"], got["blocks_per_cu_cap"]) == (key, cap), text


def test_strict_hooks_keep_their_text(dump):
    for name, field in (("FLS_FUSED_X", "x.fused_x_hook"), ("FLS_FSST_VARIANT", "x.fsst_variant_hook")):
        for text, ok in (("5", "1"), ("0", "1"), ("-1", "0"), ("5x", "0"), ("abc", "0"), ("", "0"), ("4294967296", "0")):
            got = dump({name: text})   # (atoi of a value beyond int is not checked: the launch is refused first)
            assert (got[field + ".given"], got[field + ".ok"], got[field + ".text"]) == ("1", ok, text), (name, text)
    assert check(dump, {"FLS_FUSED_FSST16": "6"})["x.fused_fsst16_given"] == "1"


def test_launch_hooks_leave_the_list_part_alone(dump):
    base = list_part(dump({}))
    envs = [{name: text} for name in LAUNCH_HOOKS for text in ("0", "1", "3", "77")]
    for env, got in zip(envs, check(dump, envs)):
        assert list_part(got) == base and got["list_is_default"] == "1", env
    # ... and beside a list hook
    keyed = {"FLS_DECODE_POLICY": "32", "FLS_STATIC_PCT": "70"}
    assert list_part(dump({**keyed, "FLS_FUSED": "0", "FLS_OVERLAP_FSST_WPC": "0"})) == list_part(dump(keyed))


def test_each_list_hook_changes_the_list_part(dump):
    base = list_part(dump({}))
    other = {"FLS_STATIC_PCT": "70", "FLS_TAIL_PIECES": "3", "FLS_BLOCKS_PER_CU": "1", "FLS_GUIDED_MIN_VECS": "1",
             "FLS_GUIDED_FACTOR": "8", "FLS_DICT_WG": "2", "FLS_DICT_WG_MIN_VECS_PER_CU": "11",
             "FLS_DICT_WG_STREAMS": "2", "FLS_DECODE_POLICY": "32", "FLS_FSST_SEG": "0"}
    assert sorted(other) == sorted(LIST_HOOKS)
    for name, text in other.items():
        got = check(dump, {name: text})
        assert list_part(got) != base and got["list_is_default"] == "0", name


HOOK_NAME = re.compile(r"FLS_(DECODE_POLICY|STATIC_PCT|TAIL_PIECES|BLOCKS_PER_CU|GUIDED_\w+|DICT_WG\w*|OVERLAP_\w+|"
                       r"FUSED\w*|FSST_SEG|FSST_SEG_CAP|FSST_VARIANT|FSST_WPC|FSST_PIECE)")


def test_every_hook_read_goes_through_the_struct():
    """No decode-launch hook is read with getenv() outside fls_tuning.hpp (a
    second parse would drift from the struct again); fls_fsst_lab.hip, the
    experiment library's own launcher, apart."""
    assert all(HOOK_NAME.fullmatch(n) for n in LIST_HOOKS + LAUNCH_HOOKS)
    bad, seen = [], set()
    for f in CSRC.glob("*"):
        for m in re.finditer(r'getenv\(\s*"(FLS_[A-Z0-9_]+)"\s*\)', f.read_text(errors="replace")):
            if not HOOK_NAME.fullmatch(m.group(1)):
                continue
            if f.name == "fls_tuning.hpp":
                seen.add(m.group(1))
            elif f.name != "fls_fsst_lab.hip":
                bad.append(f"{f.name}: {m.group(1)}")
    assert not bad, bad
    assert "FLS_BLOCKS_PER_CU" in seen   # the pattern does find the reads that are there
