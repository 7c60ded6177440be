"""The hop tier's builder (gorp_amd/csrc/gx_hop.cpp) on host-only handles: its self-check -- every run, loop set, chain element, tail
set and chain program against the dense rows -- over definitions other than the syslog family, and the preconditions of
tests/test_gpu_hop.py (which definitions have hop tables, which leave records out of LDS), so that the GPU tests cannot quietly
test other kernels.  No kernel runs here."""
import random

import numpy as np
import pytest

import hop_cases as HC
import test_compiler_vs_oracle as TC
from gorp_amd import _native as N
from gorp_amd.gorp import FlattenedExtraction, Gorp, GorpError, lines_to_csr
from oracle import oracle as O
from test_gpu_parity import oracle_for

HOP_HOST = N.GX_CREATE_HOST_ONLY | N.GX_CREATE_TIER_HOP
SIZES = [(n, seed) for n in (8, 48, 400) for seed in (1, 2, 3)]


def test_random_definitions_have_checked_hop_tables():
    """600 definitions of test_compiler_vs_oracle's generator with GX_CREATE_TIER_HOP: the builder's self-check passes on every one
    (a failure is an 'internal: hop tier ...' error from gx_create), the match automaton always has its image, the fused automaton has
    one unless its capture programs are general (reason 2) -- and at least half of the definitions have one, which is what
    test_random_definitions_through_the_hop_kernels relies on."""
    from gorp_amd.gorp import _create
    rng = random.Random(4321)
    tally, reasons = {}, {}
    n_defs = n_fused = 0
    while n_defs < 600:
        exts = [{"name": "e%d" % i, "pieces": TC.gen_pieces(rng)} for i in range(rng.randint(1, 4))]
        fl = [FlattenedExtraction(e["name"], e["pieces"]) for e in exts]

        def regexes():
            built = [f.build() for f in fl]
            return [b[0] for b in built], [b[1] for b in built]

        def product():
            try:
                return _create(*regexes(), HOP_HOST)
            except GorpError as e:
                assert "internal" not in str(e), (exts, str(e))
                raise

        pair = TC.construct_both(product, lambda: O.OracleGorp(*regexes()), tally)
        if pair is None:
            continue
        h, _ = pair
        n_defs += 1
        stat = lambda k: N.lib().gx_stat(h.ptr, k)
        reasons[stat(26)] = reasons.get(stat(26), 0) + 1
        assert stat(26) in (0, 2), (exts, stat(26))
        assert (stat(14) > 0) == (stat(26) == 0), exts
        assert stat(22) > 0, exts
        n_fused += stat(14) > 0
    print("hop tier refusals by reason:", reasons)
    assert 2 * n_fused >= n_defs, (n_fused, n_defs)
    assert tally.get("product_only", 0) == 0 and tally.get("oracle_only", 0) == 0, tally


@pytest.mark.parametrize("n,seed", SIZES)
def test_fielded_definitions_have_hop_tables(n, seed):
    """No fielded definition is refused; 400 extractions reach more states than either kernel keeps records in LDS for (the walk that
    fetches records from global memory), 48 have chains and dense rows in LDS."""
    rules, _, _ = HC.fielded(n, seed)
    g = Gorp.construct(rules, host_only=True, flags=N.GX_CREATE_TIER_HOP)
    assert g.stat(26) == 0 and g.stat(14) > 0 and g.stat(22) > 0
    if n == 400:
        assert g.stat(16) > g.stat(15) and g.stat(21) < g.stat(15)
    if n == 48:
        assert g.stat(17) > 0 and g.stat(20) > 0
        assert g.stat(16) == g.stat(15)      # (every reachable record in LDS: the all-hot walk)


@pytest.mark.parametrize("n,seed", SIZES)
def test_makers_write_lines_the_oracle_matches(n, seed):
    """The line makers themselves: at least nine of ten well-formed lines match, in the extraction they were made for where they do."""
    rules, makers, rng = HC.fielded(n, seed)
    orc = oracle_for(rules)
    for style in ("lower", "mixed"):
        picks = [rng.randrange(n) for _ in range(400)]
        lines = [makers[k](rng, style=style) for k in picks]
        data, offsets = lines_to_csr([s.encode("latin-1") for s in lines])
        mid, _ = orc.extract_batch(data, offsets, nthreads=4)
        assert 10 * int((mid >= 0).sum()) >= 9 * len(lines), (style, int((mid >= 0).sum()))
        assert 10 * int((mid == np.array(picks)).sum()) >= 9 * len(lines), style


def test_damage_and_cut_pairs():
    rng = random.Random(3)
    line = "<12>svc ab=12 cd=xyz took 7"
    out = [HC.damage(rng, line) for _ in range(400)]
    assert all(ord(ch) < 0x100 for d in out for ch in d)
    assert any(len(d) < len(line) and line.startswith(d) for d in out)            # cut short
    assert any(len(d) == len(line) and d != line for d in out)                    # one byte replaced ...
    assert any("\x00" in d for d in out) and any("\x7f" in d for d in out)       # ... by NUL, by 0x7F
    assert any("\t" in d for d in out) and any("  " in d for d in out)            # blanks tabbed, doubled
    assert any(len(d) > 2 * len(line) for d in out)                               # a stretch repeated
    assert HC.damage(rng, "") == ""
    pairs = list(HC.cut_pairs("abc"))
    assert pairs == ["", "abc", "a", "bc", "ab", "c", "abc", ""]


def test_a_definition_cannot_hold_nul_but_a_class_can_match_it():
    """Why hop_cases writes its NUL separator as a class: a definition goes to the library as C strings and would end at the NUL -- the
    Python binding refuses it on every path instead of compiling another definition -- and the class that holds nothing but U+0000 is
    a hop chain element like any other."""
    from gorp_amd.gorp import DefinitionParseException, DefinitionReader, RegexHelper, _create
    nul = FlattenedExtraction("e", [["text", "a\x00;b"]])
    for call in (lambda: RegexHelper.quoteLiteralAsRegexp("a\x00;b"), lambda: RegexHelper.massageRegexpForAutomaton("a\x00;b"),
                 lambda: RegexHelper.massageRegexpForJDK("a\x00;b"), nul.build, lambda: Gorp.construct([nul], host_only=True),
                 lambda: _create(["a\x00b"], None, N.GX_CREATE_HOST_ONLY), lambda: _create(["ab"], ["a\x00b"], N.GX_CREATE_HOST_ONLY),
                 lambda: DefinitionReader("extract e {\n   template a\x00b\n}\n", "<test>").read(host_only=True)):
        with pytest.raises(DefinitionParseException, match="U\\+0000") as ei:
            call()
        assert ei.value.code == N.GX_E_UNSUPPORTED_CONSTRUCT
    # (a differential that drew such a definition would not lose it quietly: the refusal is no ValueError, which construct_both
    # counts as the front end's, and the oracle's side raises it again, where only an OracleError is expected)
    with pytest.raises(DefinitionParseException):
        TC.construct_both(lambda: Gorp.construct([nul], host_only=True), lambda: oracle_for([nul]), {})
    rule = FlattenedExtraction("e", [["text", "a"], ["extractor", "v", [["pattern", "\\w+"]]], ["pattern", HC.NUL_CLASS], ["text", ";"],
                                     ["extractor", "n", [["pattern", "\\d+"]]]])
    g = Gorp.construct([rule], host_only=True, flags=N.GX_CREATE_TIER_HOP)
    assert g.stat(26) == 0 and g.stat(17) > 0
    orc = oracle_for([rule])
    assert orc.extract("ab\x00;12") == (0, [(1, 2), (4, 6)])
    assert orc.extract("ab;12")[0] == -1 and orc.extract("ab\x01;12")[0] == -1 and orc.extract("abĀ;12")[0] == -1
