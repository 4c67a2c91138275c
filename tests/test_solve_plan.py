"""The solver's launch rules (is-vins_amd/csrc/isv_solve_plan.h: plan_handle, plan_upload and the ISV_DEBUG_PATH formatters) on the CPU,
through the stand-alone program tests/native/solve_plan_print.cpp built under AddressSanitizer + UBSan (runtimes linked statically;
nothing is loaded into Python).  Three checks:
  a. against expected_path(), the Python restatement the GPU test asserts, for every case of tests/step_cases.py at 256 CUs;
  b. against the ISV_DEBUG_PATH lines recorded on one MI355X from the commit BEFORE the rules became a header
     (tests/golden/solve_plan_parent_lines.json): the program must reproduce them exactly -- the rules moved and did not change;
  c. the rule boundaries no GPU test reaches, each expected value derived in a comment from the formula.
The six per-handle sizes that stay beside their kernels (build_solve_sb_bytes, ...) are inputs of the rules: tests/golden/solve_plan_sizes.json
holds them as the library computes them, keyed "device frames,n_vo" (max_rollpitch = n_vo + 1, abi.make_config's default), and (b) pins
its lds_sb / lds_st entries to the recorded lines."""
import json
import os
import re
import subprocess

import pytest

from step_cases import CASES, expected_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = json.load(open(os.path.join(GOLDEN, "solve_plan_sizes.json")))
RECORDED = json.load(open(os.path.join(GOLDEN, "solve_plan_parent_lines.json")))
N_CUS = 256
REGS = 4                     # workgroups of k_dogleg<true> per CU by registers: its launch bounds (256, 4), and what the MI355X reports (recorded)


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    exe = tmp_path_factory.mktemp("solve_plan") / "solve_plan_print"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "native", "solve_plan_print.cpp"), "-o", str(exe)])

    def run(cases):
        """cases: {name: words} -> {name: dict(lines=[the four debug lines], handle={...}, upload={...})}"""
        text = "".join(f"case={name} " + " ".join(f"{k}={v}" for k, v in words.items()) + "\n" for name, words in cases.items())
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stdout + out.stderr
        res, cur = {}, None
        for line in out.stdout.splitlines():
            if line.startswith("case "):
                cur = res.setdefault(line[5:], dict(lines=[]))
            elif line.startswith("isv: "):
                cur["lines"].append(line)
            else:
                kind = re.match(r"plan: (\w+) ", line).group(1)
                cur[kind] = {k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in re.findall(r"(\w+)=(\S+)", line)}
        assert list(res) == list(cases)
        return res
    return run


def words(N, Nvo, max_lm, max_batch=1, ex=0, env=None, n_cus=N_CUS, regs=REGS, B=1, Lmax=None, Ftot=None, Fmax=None, **upload):
    """one case of the program: a handle as isv_backend_create shapes it (isv_backend.hip) and one upload"""
    Lmax = max_lm if Lmax is None else Lmax
    Fmax = 4 * Lmax if Fmax is None else Fmax
    w = dict(N=N + ex, Nr=N, est_ex=ex, n_prior_slots=2 + (Nvo - 1) + (Nvo + 1), prior_H_sz=81 + 90 * (Nvo - 1) + 27 * (Nvo + 1), max_lm=max(max_lm, 1),
             max_batch=max_batch, n_cus=n_cus, dogleg_per_cu_regs=regs, **SIZES[f"{N + ex},{Nvo}"], B=B, Lmax=Lmax, Fmax=Fmax, Ftot=B * Fmax if Ftot is None else Ftot, **upload)
    w.update(env or {})
    return w


def said(result):
    out = {}
    for line in result["lines"]:
        out.update({k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)})
    return out


# ---- a. the Python restatement -----------------------------------------------------------------------------------------------
def test_program_agrees_with_the_python_restatement(printer):
    import isvins_loader
    isvins_loader.load()
    from isvins_amd import synth
    cases, Ls = {}, {}
    for name, spec in CASES.items():
        Ls[name] = spec.get("Ls", [spec["L"]])
        # (the factor counts of the case's windows: they decide fused / control_in_wg)
        F = [synth.make_window(spec["wid"] + k, n_frames=spec["N"], n_vo=spec["Nvo"], n_landmarks=L, margin_old=0, **spec.get("make", {})).n_factors
             for k, L in enumerate(Ls[name])]
        cases[name] = words(spec["N"], spec["Nvo"], max(Ls[name]), spec.get("max_batch", 1), spec.get("ex", 0), spec.get("env", {}),
                            B=len(F), Ftot=sum(F), Fmax=max(F))
    got = printer(cases)
    for name, spec in CASES.items():
        s = said(got[name])
        assert s["lds_T"] == dict(spec.get("expect", {})).get("lds_T", 1), (name, s)
        want = expected_path(spec, s["lds_T"], len(Ls[name]), max(Ls[name]))
        assert {k: s.get(k) for k in want} == want, (name, s, want)
        if "solve_st" in spec.get("expect", {}):
            assert s["solve_st"] == spec["expect"]["solve_st"], (name, s)


# ---- b. the lines of the commit before ---------------------------------------------------------------------------------------
def test_program_reproduces_the_recorded_lines(printer):
    names = {r["name"] for r in RECORDED}
    # N = 11 and 18 at four capacities, a free extrinsic, config 5's 30 000-factor window at N = 20, N = 21, windows that split
    assert {f"n{n}_mb{b}" for n in (11, 18) for b in (1, 128, 512, 1024)} <= names and {"ex_n11", "n20_config5", "n21_dense", "split_l193", "split_l1025"} <= names
    cases = {r["name"]: words(r["N"], r["Nvo"], r["max_landmarks"], r["max_batch"], r["est_ex"], r["env"], r["n_cus"], r["dogleg_per_cu_regs"],
                              B=r["B"], Lmax=r["Lmax"], Ftot=r["Ftot"], Fmax=r["Fmax"]) for r in RECORDED}
    got = printer(cases)
    for r in RECORDED:
        assert len(r["lines"]) == 4, r
        assert got[r["name"]]["lines"] == r["lines"], (r["name"], got[r["name"]]["lines"], r["lines"])
        # the size table is what the library computes: its two entries the lines carry
        s = said(dict(lines=r["lines"][:2]))
        z = SIZES[f"{r['N'] + r['est_ex']},{r['Nvo']}"]
        assert (s["lds_sb"], s["lds"]) == (z["sb"], z["st"]), (r["name"], s, z)


# ---- c. the boundaries -------------------------------------------------------------------------------------------------------
def test_solve_st_and_chain_split_follow_the_handles_capacity(printer):
    """solve_st = fits && max_batch > per_cu_sb * n_cus, per_cu_sb = 2 up to 11 frames and 1 beyond (lds_st = 39392 <= 40 KB at N = 11,
    76224 <= 80 KB at N = 18: both fit): N = 11 flips between 2 * 256 = 512 and 513, N = 18 between 256 and 257.
    chain_split = lds_T && !solve_st && max_batch <= n_cus: flips between 256 and 257 (N = 11, where solve_st is still off there).
    ISV_SOLVE_ST / ISV_CHAIN_SPLIT = 0 | 1 force either way."""
    got = printer({"n11_512": words(11, 5, 40, 512), "n11_513": words(11, 5, 40, 513), "n18_256": words(18, 8, 40, 256), "n18_257": words(18, 8, 40, 257),
                   "n11_256": words(11, 5, 40, 256), "n11_257": words(11, 5, 40, 257),
                   "st_forced": words(11, 5, 40, 1, env=dict(ISV_SOLVE_ST=1)), "st_off": words(11, 5, 40, 1024, env=dict(ISV_SOLVE_ST=0)),
                   "cs_forced": words(11, 5, 40, 1024, env=dict(ISV_SOLVE_ST=0, ISV_CHAIN_SPLIT=1)), "cs_off": words(11, 5, 40, 1, env=dict(ISV_CHAIN_SPLIT=0))})
    st = {k: (v["handle"]["solve_st"], v["handle"]["chain_split"]) for k, v in got.items()}
    assert st == {"n11_512": (0, 0), "n11_513": (1, 0), "n18_256": (0, 1), "n18_257": (1, 0), "n11_256": (0, 1), "n11_257": (0, 0),
                  "st_forced": (1, 0), "st_off": (0, 0), "cs_forced": (0, 1), "cs_off": (0, 0)}
    assert got["n11_513"]["handle"]["SOLVE"] == "ST_N11/256/39392" and got["n18_257"]["handle"]["SOLVE"] == "ST_N18/512/76224"
    assert got["n11_257"]["handle"]["SOLVE"] == "SB_N11/512/64872" and "CHAIN" not in got["n11_257"]["handle"]
    assert got["n11_256"]["handle"]["CHAIN"] == got["n11_256"]["handle"]["POSE"] == "SB_N11/512/64872" and "SOLVE" not in got["n11_256"]["handle"]


def test_split_cap_and_the_uploads_that_split(printer):
    """split_cap = 32 while max_batch * (min(passes, 32) + 1) <= n_cus, else 1.  N = 18, 300 landmarks: passes = ceil(300 / 64) = 5, so
    max_batch * 6 <= 256: 1 -> 32, 42 (252) -> 32, 43 (258) -> 1, 64 -> 1; the scratch r1_part holds min(passes, split_cap) = 5 groups.
    An upload splits when its longest window has >= 4 passes of its own: lg_lcap = 192 -> 3 passes, no; 193 landmarks -> lg_lcap 224 -> 4, yes.
    GrMax = min(handle passes, split_cap) = 5 either way; Gs (Gram groups) is 0 for a fused upload, else clamp(n_cus / B - GrMax, 1, 16) = 16 at B = 1.
    bsub_split = split && lg_lcap > 1024: 1024 landmarks -> lg_lcap 1024, no; 1025 -> 1056, yes (then no k_pose_dogleg).
    A free extrinsic or ISV_NO_SPLIT never splits."""
    got = printer({"mb1": words(18, 8, 300, 1), "mb42": words(18, 8, 300, 42), "mb43": words(18, 8, 300, 43), "mb64": words(18, 8, 300, 64),
                   "l192": words(18, 8, 300, 1, Lmax=192), "l193": words(18, 8, 300, 1, Lmax=193),
                   "legacy": words(18, 8, 300, 1, env=dict(ISV_LEGACY_VISUAL=1)),
                   "l1024": words(11, 5, 1100, 1, Lmax=1024), "l1025": words(11, 5, 1100, 1, Lmax=1025),
                   "ex": words(11, 5, 300, 1, ex=1), "no_split": words(18, 8, 300, 1, env=dict(ISV_NO_SPLIT=1))})
    assert {k: (got[k]["handle"]["split_cap"], got[k]["handle"]["r1_groups"]) for k in ("mb1", "mb42", "mb43", "mb64")} == {"mb1": (32, 5), "mb42": (32, 5), "mb43": (1, 0), "mb64": (1, 0)}
    assert "SCHUR_SPLIT" in got["mb42"]["handle"] and "SCHUR_SPLIT" not in got["mb43"]["handle"] and "RANK1_SPLIT" not in got["mb43"]["handle"]
    assert [said(got[k])["split"] for k in ("mb1", "mb64", "l192", "l193", "ex", "no_split")] == [1, 0, 0, 1, 0, 0]
    assert (got["l193"]["upload"]["GrMax"], got["l193"]["upload"]["Gs"], got["legacy"]["upload"]["Gs"]) == (5, 0, 16)
    assert got["legacy"]["upload"]["grids"].split("/")[6:8] == ["21", "28"]        # split launch: Gs + GrMax = 21 rows; fold: nt (nt + 1) / 2 = 28 tiles at nt = 7
    assert [(said(got[k])["split"], said(got[k])["bsub_split"], said(got[k])["pose_dogleg"]) for k in ("l1024", "l1025")] == [(1, 0, 1), (1, 1, 0)]
    assert got["l1025"]["upload"]["backsub"] == "9/2640"                               # ceil(1056 / 128) = 9 groups of 128 landmarks; 2 np doubles


def test_fused_control_counts_one_resident_round_with_the_final_staging_flags(printer):
    """N = 11, n_vo = 5: 12 prior slots, prior_H_sz = 603, np = 165.  k_dogleg's LDS with the priors' J^T J record staged:
    (10 * 48 + 12 * 16 + 992 + 165 + 603) * 8 + prior_lds_bytes(12, false) + 2 * 165 * 8 = 19456 + 6960 + 2640 = 29056; unstaged 603 * 8 less: 24232.
    The step control's, lg_lcap = 128: (330 + 12 + 768) * 8 = 8880, below both.
    dg_stage_ph stays while floor(163840 / (29056 + 2304)) = 5 workgroups per CU hold the batch: 5 * 256 = 1280 windows; beyond, it drops FIRST and the
    LDS bound of the fused control is then taken from the unstaged size: floor(163840 / (24232 + 2304)) = 6 per CU.
    With 4 workgroups per CU by registers (the MI355X): resident = 256 * min(4, .) = 1024 -> fuse_control and pose_dogleg go off at B = 1025.
    With 8 by registers the LDS bound rules: B = 1281 has dropped the staging, holds 6 per CU = 1536 >= 1281 and STAYS fused (sized with the stale
    flag it would hold 1280 and lose the fused control); off at 1537."""
    env = dict(ISV_SOLVE_ST=0, ISV_CHAIN_SPLIT=1)                 # (a chain-split handle of this capacity: the one that has k_pose_dogleg)
    mk = lambda B, regs: words(11, 5, 128, 2048, env=env, regs=regs, B=B, Fmax=400)
    got = printer({"r4_1024": mk(1024, 4), "r4_1025": mk(1025, 4), "r8_1280": mk(1280, 8), "r8_1281": mk(1281, 8), "r8_1536": mk(1536, 8), "r8_1537": mk(1537, 8),
                   "split_control": words(11, 5, 128, 1, env=dict(ISV_SPLIT_CONTROL=1))})
    row = lambda k: (got[k]["upload"]["dg_stage_ph"], said(got[k])["fuse_control"], said(got[k])["pose_dogleg"], got[k]["upload"]["dogleg"])
    assert row("r4_1024") == (1, 1, 1, "NONE/29056") and row("r4_1025") == (1, 0, 0, "DOGLEG/29056")
    assert row("r8_1280") == (1, 1, 1, "NONE/29056") and row("r8_1281") == (0, 1, 1, "NONE/24232")
    assert row("r8_1536") == (0, 1, 1, "NONE/24232") and row("r8_1537") == (0, 0, 0, "DOGLEG/24232")
    assert got["r8_1281"]["upload"]["solve"] == "POSE_DOGLEG/64872" and got["r8_1537"]["upload"]["solve"] == "POSE/64872"   # max(lds_sb, 24232)
    assert got["r8_1537"]["upload"]["step_control"] == 8880 and got["r8_1537"]["upload"]["control_in_wg"] == 1
    assert row("split_control") == (1, 0, 0, "DOGLEG/29056")


def test_per_upload_flags(printer):
    """control_in_wg: Ftot <= 4096 B, or a free extrinsic (only the per-window kernels evaluate it): B = 2, 8192 factors yes, 8193 no, 8193 with an extrinsic yes.
    sw_global: more than 256 windows on a handle with the global scratch -- pair partials of n_pairs * 84 * 8 bytes > 40 KB: N = 18 (153 pairs, 102816) has it,
    N = 11 (55 pairs, 36960) has not -- or ISV_DEBUG_SW_GLOBAL.
    lgw = 8 while B <= n_cus and k_lin_gram's eight-wavefront LDS fits 160 KB: N = 18: (18 * 12 + 12 + 8 * 16 * 27 + 153 * 84 + 78 + 78 + 4 lcap) * 8
    = (16692 + 4 lcap) * 8 <= 163840 <=> lcap <= 947: lg_lcap 928 fits, 960 (929 landmarks) does not; the four-wavefront form (14964 + 4 lcap) still does: fused.
    ctl_stage_lm: 6 * lg_lcap * 8 <= 36 KB <=> lg_lcap <= 768.
    fused: not with ISV_LEGACY_VISUAL, a window above 8192 factors, or landmarks beyond the four-wavefront LDS (14964 + 4 lcap > 20480 <=> lcap > 1379);
    a free extrinsic is fused whatever else holds, or refused (N = 12 device frames ... real frames 11: (132 + 12 + 64 * 39 + 55 * 84 + 29 + 29 + 4 lcap) * 8,
    7318 + 4 lcap <= 20480 <=> lcap <= 3290)."""
    got = printer({"f8192": words(11, 5, 128, 2, B=2, Ftot=8192, Fmax=4100), "f8193": words(11, 5, 128, 2, B=2, Ftot=8193, Fmax=4100),
                   "f8193_ex": words(11, 5, 128, 2, ex=1, B=2, Ftot=8193, Fmax=4100),
                   "sw_n18_256": words(18, 8, 40, 512, B=256), "sw_n18_257": words(18, 8, 40, 512, B=257), "sw_n11_257": words(11, 5, 40, 512, B=257),
                   "sw_debug": words(11, 5, 40, 1, env=dict(ISV_DEBUG_SW_GLOBAL=1)),
                   "lgw_256": words(11, 5, 40, 512, B=256), "lgw_257": words(11, 5, 40, 512, B=257),
                   "lgw_l928": words(18, 8, 1000, 1, Lmax=928), "lgw_l929": words(18, 8, 1000, 1, Lmax=929), "lgw_hook": words(11, 5, 40, 1, env=dict(ISV_LG_BATCH_WAVES=1)),
                   "stage_768": words(11, 5, 800, 1, Lmax=768), "stage_769": words(11, 5, 800, 1, Lmax=769),
                   "long_window": words(20, 8, 1300, 1, Lmax=400, Fmax=8193), "longest_fused": words(20, 8, 1300, 1, Lmax=400, Fmax=8192),
                   "legacy": words(11, 5, 40, 1, env=dict(ISV_LEGACY_VISUAL=1)), "legacy_ex": words(11, 5, 40, 1, ex=1, env=dict(ISV_LEGACY_VISUAL=1)),
                   "lm_1376": words(18, 8, 1500, 1, Lmax=1376), "lm_1377": words(18, 8, 1500, 1, Lmax=1377),
                   "ex_3264": words(11, 5, 3400, 1, ex=1, Lmax=3264), "ex_3300": words(11, 5, 3400, 1, ex=1, Lmax=3300),
                   "resident_long": words(11, 5, 1300, 2, B=2, Ftot=8193, Fmax=4100, resident=1), "resident_ok": words(11, 5, 1300, 2, B=2, Ftot=8192, Fmax=4100, resident=1),
                   "resident_dense": words(21, 10, 40, 1, resident=1)})
    up = lambda k, f: got[k]["upload"][f]
    assert [up(k, "control_in_wg") for k in ("f8192", "f8193", "f8193_ex")] == [1, 0, 1]
    assert up("f8193", "dogleg") .startswith("DOGLEG/") and said(got["f8193"])["fuse_control"] == 0
    assert [(got[k]["handle"]["has_sw_part"], up(k, "sw_global")) for k in ("sw_n18_256", "sw_n18_257", "sw_n11_257", "sw_debug")] == [(1, 0), (1, 1), (0, 0), (1, 1)]
    assert [said(got[k])["lgw"] for k in ("lgw_256", "lgw_257", "lgw_l928", "lgw_l929", "lgw_hook")] == [8, 4, 8, 4, 4]
    assert said(got["lgw_l929"])["fused"] == 1 and up("lgw_l929", "visual") == f"LIN_GRAM/{(14964 + 4 * 960) * 8}"
    assert up("lgw_l928", "visual").startswith("LIN_GRAM_CHAIN/") and said(got["lgw_l928"])["lg_chain"] == 1
    assert [up(k, "ctl_stage_lm") for k in ("stage_768", "stage_769")] == [1, 0]
    # fused_refusal: 0 fused, 1 ISV_LEGACY_VISUAL, 2 a long window, 3 LDS, 4 / 5 resident sequences off the LDS path / above 4096 factors per window
    assert [(up(k, "fused_visual"), up(k, "fused_refusal")) for k in ("long_window", "longest_fused", "legacy", "legacy_ex", "lm_1376", "lm_1377", "ex_3264", "ex_3300")] == \
        [(0, 2), (1, 0), (0, 1), (1, 0), (1, 0), (0, 3), (1, 0), (0, 3)]
    assert [(up(k, "fused_visual"), up(k, "fused_refusal")) for k in ("resident_long", "resident_ok", "resident_dense")] == [(0, 5), (1, 0), (0, 4)]
    assert up("long_window", "visual") == "NONE/0" and said(got["long_window"])["fused"] == 0


def test_handle_kernel_forms(printer):
    """KR_LIN_GRAM_CHAIN_R1 (the rank-1 downdates inside k_lin_gram_chain) exists only for nt = (6 N + 16) / 16 = 7 tiles (N = 16 .. 18), beyond 11 frames,
    without an extrinsic and not with ISV_GENERIC_N: N = 15 -> nt 6, N = 19 -> nt 8, N = 17 with an extrinsic -> 18 device frames but EX.
    r1_dense by the LDS bound alone: N = 20: wd_ld = 128, nt = 8; panel (64 * 132 + 3 L + 2) * 8 plus lists (36 + 3) * 64 = 2496 > 163840
    <=> 3 L > 11718 <=> L >= 3907.  lds_T is decided without the lists: still 1 there.
    The compile-time window lengths: N = 11 (sb, st, k_lin_gram_chain, k_pose_dogleg) and N = 18 (st only), run-time forms with ISV_GENERIC_N."""
    got = printer({"n15": words(15, 8, 40), "n16": words(16, 8, 40), "n18": words(18, 8, 40), "n19": words(19, 8, 40), "n17_ex": words(17, 8, 40, ex=1),
                   "n18_generic": words(18, 8, 40, env=dict(ISV_GENERIC_N=1)), "n18_cs_off": words(18, 8, 40, env=dict(ISV_CHAIN_SPLIT=0)),
                   "l3906": words(20, 8, 3906), "l3907": words(20, 8, 3907), "l40_hook": words(20, 8, 40, env=dict(ISV_R1_DENSE=1)),
                   "n11": words(11, 5, 40), "n11_generic": words(11, 5, 40, env=dict(ISV_GENERIC_N=1)), "n10": words(10, 5, 40), "n11_ex": words(11, 5, 40, ex=1),
                   "n11_no_pd": words(11, 5, 40, env=dict(ISV_NO_POSE_DOGLEG=1)), "n12": words(12, 5, 40),
                   "n18_st": words(18, 8, 40, 1024), "n18_st_generic": words(18, 8, 40, 1024, env=dict(ISV_GENERIC_N=1)), "n21": words(21, 10, 40)})
    assert [said(got[k])["r1_in_lg_kernel"] for k in ("n15", "n16", "n18", "n19", "n17_ex", "n18_generic", "n18_cs_off")] == [0, 1, 1, 0, 0, 0, 0]
    assert [(said(got[k])["lds_T"], got[k]["handle"]["r1_dense"]) for k in ("l3906", "l3907", "l40_hook")] == [(1, 0), (1, 1), (1, 1)]
    assert got["l3906"]["handle"]["lds_r1"] == (64 * 132 + 3 * 3906 + 2) * 8 + 2496 == 163840 and got["l3907"]["handle"]["lds_r1"] == (64 * 132 + 3 * 3907 + 2) * 8
    h = lambda k, r: got[k]["handle"].get(r, "absent").split("/")[0]
    assert [h(k, "POSE") for k in ("n11", "n11_generic", "n10", "n11_ex", "n12")] == ["SB_N11", "SB_RT", "SB_RT", "SB_BIG", "SB_BIG"]
    assert [h(k, "LIN_GRAM_CHAIN") for k in ("n11", "n11_generic", "n10", "n11_ex", "n12")] == ["LGC_N11", "LGC_RT", "LGC_RT", "LGC_BIG", "LGC_BIG"]
    assert [h(k, "POSE_DOGLEG") for k in ("n11", "n11_generic", "n10", "n11_ex", "n11_no_pd", "n12")] == ["PD_N11", "PD_RT", "PD_RT", "absent", "absent", "absent"]
    assert [h(k, "SOLVE") for k in ("n18_st", "n18_st_generic", "n21", "n18_cs_off")] == ["ST_N18", "ST_BIG", "DENSE", "SB_BIG"]
    assert got["n18"]["handle"]["RANK1"].split("/")[1] == str(64 * 14) and got["n11"]["handle"]["RANK1"].split("/")[1] == str(64 * 15)   # nt = 7: 28 tiles, 2 per wavefront; nt = 5: 15, 1 each
    assert said(got["n21"])["fuse_control"] == 0 and got["n21"]["upload"]["solve"].startswith("SOLVE/") and got["n21"]["upload"]["dogleg"] == f"DOGLEG/{2 * 15 * 21 * 8}"


def test_tail_forms(printer):
    """k_finalize<256> (which clears the marginalisation record) and k_marg_bwd<3> by default; ISV_TAIL_ONE_WAVE: k_finalize<64> + k_marg_clear and a one-wavefront
    MargBackward; ISV_MARG_ONE_KERNEL / ISV_MARG_SPLIT force its one launch <2> / three launches.  The one-wavefront form is <2> when the HANDLE's
    max_batch > 3 n_cus = 768.  k_marg_fwd<256> up to B = 2 n_cus = 512.  initFactorGraph: no update(), no clearing, whatever the hooks.
    marg_bwd: 0 four wavefronts, 1 one launch, 2 three launches."""
    one = dict(ISV_TAIL_ONE_WAVE=1)
    got = printer({"default": words(11, 5, 40, 1024), "one_768": words(11, 5, 40, 768, env=one), "one_769": words(11, 5, 40, 769, env=one),
                   "one_kernel": words(11, 5, 40, 1, env=dict(ISV_MARG_ONE_KERNEL=1)), "marg_split": words(11, 5, 40, 1024, env=dict(ISV_MARG_SPLIT=1)),
                   "one_split": words(11, 5, 40, 1024, env=dict(ISV_TAIL_ONE_WAVE=1, ISV_MARG_SPLIT=1)),
                   "fwd_512": words(11, 5, 40, 1024, B=512), "fwd_513": words(11, 5, 40, 1024, B=513),
                   "no_update": words(11, 5, 40, 1, env=dict(ISV_DEBUG_NO_UPDATE=1)), "init": words(11, 5, 40, 1, init_mode=1), "init_one": words(11, 5, 40, 1, env=one, init_mode=1)})
    tail = lambda k: tuple(got[k]["upload"][f] for f in ("finalize_wide", "do_update", "clear_marg", "marg_bwd"))
    assert tail("default") == (1, 1, 1, 0) and tail("one_768") == (0, 1, 0, 2) and tail("one_769") == (0, 1, 0, 1)
    assert tail("one_kernel") == (1, 1, 1, 1) and tail("marg_split") == (1, 1, 1, 2) and tail("one_split") == (0, 1, 0, 2)
    assert tail("no_update")[:3] == (1, 0, 1) and tail("init")[:3] == (1, 0, 0) and tail("init_one")[:3] == (0, 0, 0)
    assert [got[k]["upload"]["marg_fwd_wide"] for k in ("fwd_512", "fwd_513")] == [1, 0]
