"""The feature-exclusion table (masters_thesis_amd.compat) against a recording of what the code refused before the table
existed: tests/data/refusal_matrix.json, written by tools/refusal_matrix.py at commit 4dbc1c8, whose refusals were
imperative code spread over the models and dp.attach.  The same tool runs the same cases here, on the CPU over the mock
backend; nothing below is a tolerance."""
import importlib.util
import os

import pytest

from masters_thesis_amd import compat

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("refusal_matrix", os.path.join(os.path.dirname(HERE), "tools", "refusal_matrix.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

RECORDED = tool.load(os.path.join(HERE, "data", "refusal_matrix.json"))

# Where two sites disagreed on when a feature counts as on, the table keeps the widest reading: these cases passed before
# and are refused now.  case -> the text now raised
UNIFIED = {
    # train_step_sam asked "is the decay table built" (seg_wd), so a first step that was the sharpness-aware one ran its
    # undecayed update on a decaying optimizer; dp.attach and enable_agc asked the optimizer too, and so does the table
    "attention|weight_decay:opt|sam:train_step_sam":
        compat.WEIGHT_DECAY_REFUSAL.format(what="train_step_sam"),
    # a grad_sync hook handed to the constructor was refused there beside attention_coverage, init_state, semantic and the
    # input corruption, but only by the first train_step beside these three: the constructor now refuses it beside all
    "dense|dp:ctor_hook|scheduled_sampling:ctor": "scheduled sampling has no data-parallel schedule: train it on one device",
    "attention|dp:ctor_hook|scheduled_sampling:ctor": "scheduled sampling has no data-parallel schedule: train it on one device",
    "dense|dp:ctor_hook|self_critical:ctor": "self-critical training has no data-parallel schedule: train it on one device",
    "attention|dp:ctor_hook|free_running:ctor": "the free-running step (teacher_forcing=False) has no data-parallel schedule",
}
# The same refusal, earlier: gradient_accumulation_steps assigned behind compile was found by the optimizer-state build,
# behind the step's staging launch; train_step's own check now finds it in front of every launch
CLEANER = {f"{kind}|{feature}:ctor|grad_accum:assign@3" for kind, feature in (
    ("dense", "scheduled_sampling"), ("dense", "self_critical"), ("dense", "semantic"), ("attention", "scheduled_sampling"),
    ("attention", "free_running"), ("attention", "attention_coverage"), ("attention", "init_state"))}


@pytest.fixture(scope="module")
def now():
    return tool.record()


def test_the_same_cases_exist(now):
    assert sorted(now) == sorted(RECORDED)
    assert len(RECORDED) > 400 and sum(v != "ok" for v in RECORDED.values()) > 400


@pytest.mark.parametrize("case", sorted(RECORDED))
def test_case_equals_the_recording(case, now):
    """the recorded outcome: exception class, full text, and whether the refused call left state and launches alone"""
    was, got = RECORDED[case], now[case]
    if case in UNIFIED:
        assert was == "ok" and got == {"error": ["NotImplementedError", UNIFIED[case]], "clean": got["clean"]}
        assert got["clean"] is not False
    elif case in CLEANER:
        assert was["clean"] is False and got == dict(was, clean=True)
    else:
        assert got == was


# ---------------------------------------------------------------------------------------------------- coverage of the table
CLASSES = ("NIC", "NICfc", "CaptionGenerator")
# the tool's feature names are the table's, but for the one it cannot tell apart from outside, and where one setting is two features: a world
# of two (the tool's hook, dp.attach(world=2)) is data parallel and more than one rank, normalise="weights" a token weighting
TABLE_KEYS = {"distillation": ("distillation", "distill_loss"), "dp": ("dp", "dp_multi"), "dp_multi": ("dp", "dp_multi"),
              "normalise_weights": ("normalise_weights", "token_weights")}


def _row_of(error, keys):
    """the index of the row a recorded refusal is, among the rows between the case's features ``keys`` (several rows may
    share a text), or None"""
    cls, text = error
    for i, r in enumerate(compat.ROWS):
        if r.exc.__name__ != cls or not all(k in keys or k.startswith("no_") for k in (r.a, r.b)):
            continue
        for t in (r.text, r.text_b):
            if t is None:
                continue
            forms = {t.replace("{cls}", c).replace("{sam}", s) for c in CLASSES for s in ("train_step_sam", "train_step_SAM")}
            if text in forms:
                return i
    return None


def _parse(case):
    kind, *ways = case.split("|")
    return kind, [w.split(":")[0] for w in ways], [w.split(":")[1] for w in ways]


def _stage(way):
    return {"ctor": 0, "ctor_scan": 0, "ctor_word": 0, "ctor_hook": 0, "loss": 2, "opt": 2, "class_weight": 2, "focal": 2,
            "compile_freeze": 2}.get(way, int(way.split("@")[1]) if "@" in way else 5)


def _arrivals(case):
    """the table keys that arrive with the last call of a case: the last feature, and the first one too where one call
    (one constructor, one compile) brings both"""
    kind, feats, ways = _parse(case)
    last = {feats[-1]}
    if len(feats) == 2 and _stage(ways[0]) == _stage(ways[1]) and _stage(ways[0]) in (0, 2):
        last.add(feats[0])
    return {k for f in last for k in TABLE_KEYS.get(f, (f,))}


# a direction of a row (the key that arrives last, the other being on) which the tool reaches and which raises another
# row, or nothing -- one by one, with the reason
_LATE = ("the parent's constructor took a grad_sync hook beside it and the first train_step refused (the cases of UNIFIED): "
         "the recording holds this direction as the hook attached behind compile")
EXEMPT = {
    ("free_running", "dp", "free_running"): _LATE,
    ("scheduled_sampling", "dp", "scheduled_sampling"): _LATE,
    ("self_critical", "dp", "self_critical"): _LATE,
}
# a recorded refusal of two features that is no row of the table: (class, start of the text) -> why it is none
NOT_A_PAIR = {
}


def test_every_row_is_recorded_in_every_direction_a_public_call_reaches():
    hit, reachable, stray = set(), set(), set()
    for case, v in RECORDED.items():
        arr = _arrivals(case)
        kind, feats, _ = _parse(case)
        keys = {k for f in feats for k in TABLE_KEYS.get(f, (f,))}
        for i, r in enumerate(compat.ROWS):
            for side, other in ((r.a, r.b), (r.b, r.a)):
                if side in arr and (other in keys or other.startswith("no_")):
                    reachable.add((i, side))
        if v != "ok":
            i = _row_of(v["error"], keys)
            if i is not None:
                hit |= {(i, side) for side in (compat.ROWS[i].a, compat.ROWS[i].b) if side in arr}
            elif len(feats) == 2:
                stray.add((v["error"][0], next((k for k in NOT_A_PAIR if v["error"][1].startswith(k)), v["error"][1])))
    assert {text for _, text in stray} == set(NOT_A_PAIR), sorted(stray)
    rows_hit = {i for i, _ in hit}
    assert rows_hit == set(range(len(compat.ROWS))), [compat.ROWS[i][:2] for i in set(range(len(compat.ROWS))) - rows_hit]
    missing = {(compat.ROWS[i].a, compat.ROWS[i].b, side) for i, side in reachable - hit}
    assert missing == set(EXEMPT), (sorted(missing - set(EXEMPT)), sorted(set(EXEMPT) - missing))
    assert len(EXEMPT) * 10 < len(compat.ROWS)


# a pair refused when the second feature arrives behind the first and accepted the other way round, with the reason
_WORLD_1 = ("enable_agc refuses a world of more than one rank (dp_multi): a hook without a world, or dp.attach(world=1), "
            "beside AGC is allowed, and dp.attach(world=2) behind enable_agc is refused -- that is the other order")
_NO_DESCRIPTOR = ("set_teacher on a weighted model without a distillation descriptor only holds the teacher: its step does "
                  "not distil; the compile loss that asks for both is refused")
ONE_WAY = {
    ("dense", "dp", "agc"): _WORLD_1,
    ("attention", "dp", "agc"): _WORLD_1,
    ("dense", "distillation", "token_weights"): _NO_DESCRIPTOR,
    ("attention", "distillation", "token_weights"): _NO_DESCRIPTOR,
}


def test_a_pair_refused_in_one_order_is_refused_in_the_other():
    refused, accepted = {}, {}
    for case, v in RECORDED.items():
        kind, feats, ways = _parse(case)
        if len(feats) != 2 or (_stage(ways[0]) == _stage(ways[1]) and _stage(ways[0]) in (0, 2)):
            continue
        (accepted if v == "ok" else refused).setdefault((kind, feats[0], feats[1]), []).append(case)
    one_way = {(k, a, b) for (k, a, b) in refused if (k, b, a) in accepted and (k, b, a) not in refused}
    assert one_way == set(ONE_WAY), (sorted(one_way - set(ONE_WAY)), sorted(set(ONE_WAY) - one_way))


def test_every_row_names_two_features_and_the_step_lists_are_features():
    from masters_thesis_amd.lc_nic import NIC as LcNIC
    from masters_thesis_amd.nic import NIC
    for r in compat.ROWS:
        assert r.a in compat.FEATURES and r.b in compat.FEATURES and r.a != r.b
    pairs = [frozenset((r.a, r.b)) for r in compat.ROWS]
    assert len(set(pairs)) == len(pairs)                                    # each unordered pair is one row
    for cls in (NIC, LcNIC):
        assert set(cls.STEP_FEATURES) <= set(compat.FEATURES)


def test_design_md_holds_the_table_as_the_tool_prints_it():
    with open(os.path.join(os.path.dirname(HERE), "DESIGN.md")) as f:
        assert tool.markdown() in f.read()
