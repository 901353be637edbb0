"""Per-query filters of the index search, host side (no device): `search.resolve_admit` against a brute-force set computation, the
`batch` file parser, and the command line's parser."""
import json
import random

import numpy as np
import pytest
import torch

from sprc_amd import search as S

N = 57
NAMES = [f"img-{i:03d}" for i in range(N)]
ROW_OF = {n: i for i, n in enumerate(NAMES)}


def _brute(within, exclude, within_each, exclude_each, skip_rows, removed, B):
    """Query b's set with Python sets, from rows or names -> list of B sets of rows."""
    def rows(x):
        return set(range(N)) if x is None else {ROW_OF[i] if isinstance(i, str) else int(i) for i in (x.tolist() if isinstance(x, torch.Tensor) else x)}

    def names(x):
        return set() if x is None else {ROW_OF[n] for n in x}
    out = []
    for b in range(B):
        s = rows(within) & rows(None if within_each is None else within_each[b])
        s -= names(exclude) | names(None if exclude_each is None else exclude_each[b]) | set(removed)
        if skip_rows is not None and skip_rows[b] is not None and skip_rows[b] >= 0:
            s.discard(skip_rows[b])
        out.append(s)
    return out


def _check(rows, admit, sets):
    assert rows.dtype == torch.int32 and admit.dtype == torch.int32 and rows.shape == admit.shape and rows.dim() == 1
    r = rows.tolist()
    assert r == sorted(set().union(*sets))                                         # ascending, de-duplicated, exactly the union
    words = admit.numpy().view(np.uint32).tolist()
    for m, row in enumerate(r):
        assert words[m] == sum(1 << b for b, s in enumerate(sets) if row in s), (m, row)


def _draw(rng, B, as_rows):
    def pick(lo, hi):
        chosen = sorted(rng.sample(range(N), rng.randint(lo, hi)))
        if as_rows:
            return torch.tensor(chosen) if rng.random() < 0.5 else chosen
        out = [NAMES[i] for i in chosen]
        rng.shuffle(out)
        return out + out[:2]                                                       # names may repeat and come in any order
    within = None if rng.random() < 0.3 else pick(30, N)
    exclude = [NAMES[i] for i in rng.sample(range(N), rng.randint(0, 4))]
    within_each = [None if rng.random() < 0.25 else pick(12, 40) for _ in range(B)]
    exclude_each = [None if rng.random() < 0.3 else [NAMES[i] for i in rng.sample(range(N), rng.randint(0, 5))] for _ in range(B)]
    skip = [rng.choice([-1, None, rng.randrange(N)]) for _ in range(B)]
    removed = set(rng.sample(range(N), rng.randint(0, 3)))
    return within, exclude, within_each, exclude_each, skip, removed


@pytest.mark.parametrize("B", [1, 2, 31, 32])
@pytest.mark.parametrize("as_rows", [False, True])
def test_resolve_admit_matches_brute_force(B, as_rows):
    rng = random.Random(100 * B + as_rows)
    done = 0
    for _ in range(40):
        args = _draw(rng, B, as_rows)
        sets = _brute(*args, B)
        if not all(sets):
            with pytest.raises(ValueError, match=rf"query {[bool(s) for s in sets].index(False)}:"):
                S.resolve_admit(N, ROW_OF, *args)
            continue
        _check(*S.resolve_admit(N, ROW_OF, *args), sets)
        done += 1
    assert done >= 10


def test_resolve_admit_bit_31_is_the_sign_bit():
    each = [["img-000"]] * 31 + [["img-000", "img-005"]]
    rows, admit = S.resolve_admit(N, ROW_OF, None, (), each, None, None, ())
    assert rows.tolist() == [0, 5] and admit.tolist() == [-1, -2 ** 31]
    rows, admit = S.resolve_admit(N, ROW_OF, None, (), [["img-009", "img-003", "img-009"]], None, None, ())
    assert rows.tolist() == [3, 9] and admit.tolist() == [1, 1]                     # B = 1


def test_resolve_admit_none_entries_and_interplay():
    # only exclusions: every row but those each query drops; the union is the whole gallery minus what all queries drop
    rows, admit = S.resolve_admit(N, ROW_OF, None, ["img-001"], None, [None, ["img-002"]], [3, -1], {4})
    assert rows.tolist() == [n for n in range(N) if n not in (1, 4)]
    words = dict(zip(rows.tolist(), admit.tolist()))
    assert words[0] == 3 and words[2] == 1 and words[3] == 2 and 1 not in words and 4 not in words
    # within & within_each, a None entry beside a list, skip_rows alone giving the number of queries
    rows, admit = S.resolve_admit(N, ROW_OF, ["img-010", "img-011", "img-012"], (), [None, ["img-012", "img-040", "img-011"]], None, None, ())
    assert rows.tolist() == [10, 11, 12] and admit.tolist() == [1, 3, 3]
    rows, admit = S.resolve_admit(N, ROW_OF, [5, 6], (), None, None, [6, None, -1], ())
    assert rows.tolist() == [5, 6] and admit.tolist() == [7, 6]
    # a skipped or removed row that no query lists changes nothing
    a = S.resolve_admit(N, ROW_OF, None, (), [[7, 8]], None, [30], {31})
    assert a[0].tolist() == [7, 8] and a[1].tolist() == [1, 1]


def test_resolve_admit_errors():
    ok = [["img-001"], ["img-002"]]
    with pytest.raises(KeyError):
        S.resolve_admit(N, ROW_OF, None, (), [["img-001"], ["nope"]], None, None, ())
    with pytest.raises(KeyError):
        S.resolve_admit(N, ROW_OF, ["nope"], (), ok, None, None, ())
    with pytest.raises(KeyError):
        S.resolve_admit(N, ROW_OF, None, ["nope"], ok, None, None, ())
    with pytest.raises(KeyError):
        S.resolve_admit(N, ROW_OF, None, (), ok, [None, ["nope"]], None, ())
    for bad in ([3, 1], [0, N], [-1, 2], [2, 2], torch.tensor([[1, 2]]), torch.tensor([1.0, 2.0])):
        with pytest.raises(ValueError):
            S.resolve_admit(N, ROW_OF, None, (), [[1], bad], None, None, ())
        with pytest.raises(ValueError):
            S.resolve_admit(N, ROW_OF, bad, (), ok, None, None, ())
    with pytest.raises(ValueError, match="query 1:"):
        S.resolve_admit(N, ROW_OF, None, (), ok, [None, ["img-002"]], None, ())
    with pytest.raises(ValueError, match="query 33:"):                             # the block's place in a longer call
        S.resolve_admit(N, ROW_OF, None, (), ok, None, [-1, 2], (), first=32)
    with pytest.raises(ValueError, match="query 0:"):
        S.resolve_admit(N, ROW_OF, None, (), [[]], None, None, ())
    with pytest.raises(ValueError, match="query 0:"):
        S.resolve_admit(N, ROW_OF, ["img-001"], (), ok, None, None, {1})
    with pytest.raises(ValueError):
        S.resolve_admit(N, ROW_OF, None, (), ok, [None], None, ())                 # lengths disagree
    with pytest.raises(ValueError):
        S.resolve_admit(N, ROW_OF, None, (), ok, None, [1, 2, 3], ())
    with pytest.raises(ValueError):
        S.resolve_admit(N, ROW_OF, None, (), None, None, None, ())                 # no per-query argument: how many queries?
    with pytest.raises(ValueError):
        S.resolve_admit(N, ROW_OF, None, (), [[1]] * 33, None, None, ())           # a block is at most 32 queries


class _NoDevice:
    """A Searcher whose host state is set by hand: any device call of `_search_each` would fail on the missing model."""
    def __new__(cls):
        s = S.Searcher.__new__(S.Searcher)
        s.names, s._removed, s._raw = list(NAMES), set(), S._RawRows(None, dict(ROW_OF))

        class M:
            device = "cpu"
        s.model = M()
        return s


def test_searcher_raises_before_any_device_call():
    s = _NoDevice()
    ids = torch.zeros((2, 4), dtype=torch.long)
    with pytest.raises(ValueError, match="within_each"):
        s.search_ids(["img-001", "img-002"], ids, ids, 5, within_each=[None])
    with pytest.raises(ValueError, match="exclude_each"):
        s.search_ids(["img-001", "img-002"], ids, ids, 5, exclude_each=[None] * 3)
    with pytest.raises(ValueError, match="query 1:"):
        s.search_ids(["img-001", "img-002"], ids, ids, 5, within_each=[None, ["img-002"]], exclude_reference=True)
    with pytest.raises(KeyError):
        s.search_ids(["img-001", "img-002"], ids, ids, 5, within_each=[None, ["nope"]])
    ids40 = torch.zeros((40, 4), dtype=torch.long)
    with pytest.raises(ValueError, match="query 35:"):                             # the second block of 32
        s.search_ids(["img-001"] * 40, ids40, ids40, 5, exclude_each=[None] * 35 + [NAMES] + [None] * 4)


# ---- the batch file ---------------------------------------------------------------------------------------------------------------
def test_parse_queries():
    text = "\n".join([
        json.dumps({"reference": "img-001", "caption": "a"}),
        "",
        "   ",
        json.dumps({"reference_image": "/x/y.png", "caption": "b", "within": ["img-002", "img-003"], "within_glob": "img-00*",
                    "exclude": ["img-003"], "exclude_reference": True}),
    ]) + "\n"
    got = S.parse_queries(text)
    assert [e["line"] for e in got] == [1, 4]                                      # blank lines are skipped, the numbering is the file's
    assert got[0] == dict(line=1, reference="img-001", reference_image=None, caption="a", within=None, within_glob=None, exclude=None,
                          exclude_reference=False)
    assert got[1] == dict(line=4, reference=None, reference_image="/x/y.png", caption="b", within=["img-002", "img-003"],
                          within_glob="img-00*", exclude=["img-003"], exclude_reference=True)
    good = json.dumps({"reference": "img-001", "caption": "a"})
    for bad in ('{"reference": "img-001", "caption": ', json.dumps({"reference": "img-001"}), json.dumps({"caption": "a"}),
                json.dumps({"reference": "img-001", "reference_image": "f.png", "caption": "a"}), json.dumps(["reference"]),
                json.dumps({"reference": "img-001", "caption": 3}), json.dumps({"reference": "img-001", "caption": "a", "within": "img-002"}),
                json.dumps({"reference": "img-001", "caption": "a", "exclude_reference": "yes"}),
                json.dumps({"reference": "img-001", "caption": "a", "witin": []})):
        with pytest.raises(ValueError, match="line 3:"):
            S.parse_queries(good + "\n\n" + bad + "\n" + good + "\n")
    assert S.parse_queries("") == [] and S.parse_queries("\n\n") == []


def test_query_filters():
    def entry(**kw):
        return S.parse_queries(json.dumps(dict({"reference": "img-001", "caption": "a"}, **kw)))[0]
    assert S.query_filters(entry(), NAMES, ROW_OF) == (None, None)
    assert S.query_filters(entry(exclude_reference=True), NAMES, ROW_OF) == (None, ["img-001"])
    e = S.parse_queries(json.dumps({"reference_image": "f.png", "caption": "a", "exclude_reference": True}))[0]
    assert S.query_filters(e, NAMES, ROW_OF) == (None, None)                       # a file is no gallery name: nothing to leave out
    assert S.query_filters(entry(within=["img-002", "img-020"], exclude=["img-005"]), NAMES, ROW_OF) == (["img-002", "img-020"], ["img-005"])
    assert S.query_filters(entry(within_glob="img-00?"), NAMES, ROW_OF)[0] == NAMES[:10]
    assert S.query_filters(entry(within=["img-020", "img-002"], within_glob="img-00*"), NAMES, ROW_OF)[0] == ["img-002"]
    two = json.dumps({"reference": "img-001", "caption": "a"}) + "\n"
    for bad, err in (({"within": ["img-002", "nope"]}, KeyError), ({"exclude": ["nope"]}, KeyError), ({"reference": "nope"}, KeyError),
                     ({"within_glob": "zzz*"}, ValueError)):
        e = S.parse_queries(two + json.dumps(dict({"reference": "img-001", "caption": "a"}, **bad)))[1]
        with pytest.raises(err, match="line 2:"):
            S.query_filters(e, NAMES, ROW_OF)


def test_command_line_parser():
    p = S._parser()
    a = p.parse_args(["batch", "--index", "s.safetensors", "--model-path", "m.pt", "--queries", "q.jsonl"])
    assert (a.command, a.index, a.queries, a.k, a.batch, a.out, a.dtype, a.vit_depth) == ("batch", "s.safetensors", "q.jsonl", 10, 32, None, "fp16", None)
    a = p.parse_args(["batch", "--index", "s", "--model-path", "m", "--queries", "q", "-k", "5", "--batch", "2", "--out", "o.jsonl", "--dtype", "bf16"])
    assert (a.k, a.batch, a.out, a.dtype) == (5, 2, "o.jsonl", "bf16")
    for missing in (["--index", "s", "--model-path", "m"], ["--queries", "q", "--model-path", "m"]):
        with pytest.raises(SystemExit):
            p.parse_args(["batch"] + missing)
    for n in (0, 33):
        a = p.parse_args(["batch", "--index", "s", "--model-path", "m", "--queries", "q", "--batch", str(n)])
        with pytest.raises(ValueError, match="--batch"):
            S.batch_index(a)                                                       # refused before the file or the model is touched
    # `query` parses what it parsed before
    q = p.parse_args(["query", "--index", "s", "--model-path", "m", "--reference", "r", "--caption", "c"])
    assert vars(q) == dict(command="query", index="s", reference="r", reference_image=None, caption="c", k=10, json=False, within_file=None,
                           within_glob=None, exclude=None, exclude_reference=False, model_path="m", backbone="pretrain", dtype="fp16",
                           gpu_preprocess=False, vit_depth=None)
    q = p.parse_args(["query", "--index", "s", "--model-path", "m", "--reference-image", "f.png", "--caption", "c", "-k", "3", "--json",
                      "--within-glob", "a*", "--exclude", "x", "y", "--exclude-reference"])
    assert (q.reference, q.reference_image, q.k, q.json, q.within_glob, q.exclude, q.exclude_reference) == (None, "f.png", 3, True, "a*", ["x", "y"], True)
    with pytest.raises(SystemExit):
        p.parse_args(["query", "--index", "s", "--model-path", "m", "--caption", "c"])
