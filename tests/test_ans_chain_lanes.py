"""The lane-per-chain protocol of the rANS chain kernel (csrc/jxg_ans.hip
ans_chain) restated in Python and checked against the sequential encoder, in
the style of test_ans_lane_model.py: a toy rANS step (the kernel's arithmetic
is checked on the GPU against the oracle); what this pins is which lane codes
which record at which step, what the stages hold, and where the outputs go.

A workgroup takes 64 consecutive entries of the longest-first order; lane c
of its chain wave runs chain c alone, record n_c - 1 - t at step t, and the
idle step (f = 4096) once past its record 0.  Steps run in blocks of BLK; the
chain wave only reads a stage of records and writes a stage of pre-step
states (two slots each, reused as in the kernel), and the helpers turn a
finished block's states into outputs: the emitted bits of record i at
position i, and the chain's final state = the state before its first idle
step (an empty chain: the initial state).  The workgroup runs max(n) + 1 steps, rounded up to whole blocks, so that every
chain's first idle step exists."""
import random

import pytest

INIT = 0x130000
BLK = 64
DUMMY = (4096, 0)  # the idle record: never emits (x < 2^32), any state stays valid


def step(x, rec):
    """toy rANS step: rec = (f, cum); emits the low 16 bits when x >= f << 20"""
    f, cum = rec
    out = None
    if x >= (f << 20):
        out = x & 0xFFFF
        x >>= 16
    return (x // f) * 4096 + cum + x % f, out


def sequential(recs):
    """the chain as the format defines it: records n - 1 .. 0"""
    x, outs = INIT, [None] * len(recs)
    for i in range(len(recs) - 1, -1, -1):
        x, outs[i] = step(x, recs[i])
    return x, outs


def emitted(X, rec):
    f, _ = rec
    return X & 0xFFFF if X >= (f << 20) else None


def workgroup(chains, helpers_first=True):
    """ans_chain for one workgroup: chains = up to 64 record lists (lanes
    beyond them hold no chain).  Returns per chain (final state, outputs).

    The two stages have two slots each, reused as the kernel reuses them.  In
    the loop's pass b the chain wave reads ea[b & 1] and writes x[b & 1], while
    the helpers, in this order, take block b - 1 out of x and ea, stage block
    b + 1 into ea (the slot block b - 1 just left) from the records fetched a
    pass earlier, fetch block b + 2, and turn block b - 1 into outputs.  One
    barrier ends the pass, so within it the two sides may run in either order:
    helpers_first picks one."""
    assert len(chains) <= 64
    n = [len(c) for c in chains] + [0] * (64 - len(chains))
    have = [c < len(chains) for c in range(64)]
    T = max(n) + 1
    nb = (T + BLK - 1) // BLK
    state = [INIT] * 64  # the chain wave's registers
    outs = [[None] * n[c] for c in range(64)]
    final = [None] * 64
    wrote = set()
    ea = [None, None]  # record stage slots: [step][lane]
    xst = [None, None]  # pre-step state slots

    def fetch(b):  # the helpers' registers: block b's records, idle past record 0
        return [[chains[c][n[c] - 1 - t] if have[c] and n[c] - 1 - t >= 0 else DUMMY
                 for c in range(64)] for t in range(b * BLK, (b + 1) * BLK)]

    def chain_block(b):
        nonlocal state
        xs = []
        for s in range(BLK):
            xs.append(list(state))
            state = [step(state[c], ea[b & 1][s][c])[0] for c in range(64)]
        xst[b & 1] = xs

    def flush(b, X, RC):
        for s in range(BLK):
            for c in range(64):
                i = n[c] - 1 - (b * BLK + s)
                if i >= 0:
                    assert (c, i) not in wrote
                    wrote.add((c, i))
                    outs[c][i] = emitted(X[s][c], RC[s][c])
                elif i == -1 and have[c]:
                    assert final[c] is None
                    final[c] = X[s][c]

    R = fetch(0)
    ea[0] = R
    R = fetch(1)
    for b in range(nb):
        if not helpers_first:
            chain_block(b)
        X = RC = None
        if b > 0:  # unstage before the slot is refilled
            X, RC = xst[(b - 1) & 1], ea[(b - 1) & 1]
        ea[(b + 1) & 1] = R
        R = fetch(b + 2)
        if b > 0:
            flush(b - 1, X, RC)
        if helpers_first:
            chain_block(b)
    flush(nb - 1, xst[(nb - 1) & 1], ea[(nb - 1) & 1])
    assert all(final[c] is None for c in range(64) if not have[c])  # they write nothing
    return [(final[c], outs[c]) for c in range(len(chains))]


def rand_stream(rng, n):
    out = []
    for _ in range(n):
        f = rng.choice([1, 2, 7, 64, 300, 1500, 4000, 4096])
        out.append((f, rng.randrange(0, 4097 - f)))
    return out


def frame(lengths, seed, helpers_first=True):
    """a frame's chains through the kernel's mapping: longest-first order,
    64 chains per workgroup; returns the results in the original order"""
    rng = random.Random(seed)
    chains = [rand_stream(rng, n) for n in lengths]
    order = sorted(range(len(chains)), key=lambda i: -len(chains[i]))  # stable, as the host's
    got = [None] * len(chains)
    for w in range(0, len(order), 64):
        slots = order[w:w + 64]
        for slot, res in zip(slots, workgroup([chains[i] for i in slots], helpers_first)):
            got[slot] = res
    return chains, got


MIXED = [0, 1, 63, 64, 65, 200]
CASES = {
    "all_empty": [0] * 64,
    "mixed_full_wave": (MIXED * 11)[:64],
    "fewer_than_64": MIXED + [BLK - 1, BLK, BLK + 1, 2 * BLK - 1, 2 * BLK, 5 * BLK + 3],
    "two_waves_65": [(7 * i) % 131 for i in range(65)],
    "two_waves_70": [(11 * i) % 197 for i in range(64)] + MIXED,
}


@pytest.mark.parametrize("helpers_first", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_lane_per_chain_protocol(name, helpers_first):
    lengths = CASES[name]
    chains, got = frame(lengths, len(name) * 1000 + len(lengths), helpers_first)
    for recs, res in zip(chains, got):
        assert res == sequential(recs)


def test_empty_chain_state_and_block_edges():
    """an empty chain's final state is the initial one; chains that end on the
    last step of a block take their final state from the next block"""
    chains, got = frame([0, BLK, BLK - 1, 2 * BLK], 5)
    assert got[0] == (INIT, [])
    for recs, res in zip(chains, got):
        assert res == sequential(recs)
