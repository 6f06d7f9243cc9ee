"""CPU checks of the four-outputs-per-window tables of the 7- and 9-tap stride-2 layers (tools/gen_wino1d.py: Wino4K7S2, Wino4K9S2 of
demon_amd/csrc/wino1d_tables.h; conv_wino4.hip kinds 2 and 3): polyphase F(4,4) + F(4,3) and F(4,5) + F(4,4) on the points
0, +-1, +-2, 1/2 (, -1/2), infinity.  Exact rational arithmetic, no GPU."""
import importlib.util
import os
import random
from fractions import Fraction as Fr

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# taps -> (struct, products per four outputs, window)
FORMS = {7: ("Wino4K7S2", 13, 13), 9: ("Wino4K9S2", 15, 15)}


def _gen():
    spec = importlib.util.spec_from_file_location("gen_wino1d", os.path.join(ROOT, "tools", "gen_wino1d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tables(gen, taps):
    AT, G, BT, win = gen.kind_matrices4(taps, 2)
    AT, G = gen.normalise(AT, G)
    return AT, G, BT, win


@pytest.mark.parametrize("taps", sorted(FORMS))
def test_identity_holds_exactly_in_rationals(taps):
    """AT [(G g) . (BT d)] = the stride-2 correlation of d with g, for rational operands (not only the integers of gen.check)"""
    gen = _gen()
    AT, G, BT, win = _tables(gen, taps)
    gen.check(AT, G, BT, taps, 2, win)
    rnd = random.Random(11)
    for _ in range(25):
        d = [Fr(rnd.randint(-50, 50), rnd.randint(1, 9)) for _ in range(win)]
        g = [Fr(rnd.randint(-50, 50), rnd.randint(1, 9)) for _ in range(taps)]
        U = [sum(G[e][t] * g[t] for t in range(taps)) for e in range(len(G))]
        T = [sum(BT[e][n] * d[n] for n in range(win)) for e in range(len(G))]
        Y = [sum(AT[k][e] * U[e] * T[e] for e in range(len(G))) for k in range(4)]
        assert Y == [sum(d[2 * k + t] * g[t] for t in range(taps)) for k in range(4)]


@pytest.mark.parametrize("taps", sorted(FORMS))
def test_weight_and_input_transforms_are_integer(taps):
    gen = _gen()
    AT, G, BT, win = _tables(gen, taps)
    assert all(v.denominator == 1 for row in G for v in row)
    assert all(v.denominator == 1 for row in BT for v in row)
    # the figures the kernels' exact checks rely on: small integers (fp32 holds their products with the test operands exactly) and
    # the smallest non-zero |AT| entry, which an integer error in one accumulator moves an output by
    assert max(abs(v) for row in G for v in row) == {7: 8, 9: 16}[taps]
    assert max(abs(v) for row in BT for v in row) == {7: 12, 9: 21}[taps]
    assert min(abs(v) for row in AT for v in row if v) == {7: Fr(1, 120), 9: Fr(1, 360)}[taps]
    assert max(sum(1 for v in row if v) for row in AT) == {7: 11, 9: 13}[taps]


@pytest.mark.parametrize("taps", sorted(FORMS))
def test_products_per_four_outputs(taps):
    gen = _gen()
    AT, G, BT, win = _tables(gen, taps)
    name, nuv, want_win = FORMS[taps]
    assert len(AT) == 4 and len(G) == len(BT) == nuv and all(len(row) == nuv for row in AT)
    assert win == want_win == 2 * 4 + taps - 2 and all(len(row) == win for row in BT) and all(len(row) == taps for row in G)
    assert Fr(nuv, 4 * taps) == {7: Fr(13, 28), 9: Fr(15, 36)}[taps]   # of the direct form's multiply-adds


def test_committed_header_is_current_and_has_both_structs():
    gen = _gen()
    text = gen.render()
    with open(gen.HEADER) as f:
        assert f.read() == text, "demon_amd/csrc/wino1d_tables.h is stale: run python tools/gen_wino1d.py"
    for taps, (name, nuv, win) in FORMS.items():
        assert "struct %s {" % name in text
        assert "static constexpr int TAPS = %d, STRIDE = 2, NUV = %d, WIN = %d, OUT = 4;" % (taps, nuv, win) in text
