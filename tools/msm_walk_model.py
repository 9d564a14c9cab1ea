#!/usr/bin/env python3
"""Cost model of the Pippenger bucket walk (k_msm_buckets, hbtc_msm.hip) in Fq products per lane.

For random scalars it restates what the kernels do -- k_msm_recode's signed c-bit digits, k_msm_sort's
order (largest bucket first), the equal slices of the sorted list over S = B/8 segment lanes, 64
consecutive (msm, window, segment) lanes per wave -- and counts, per lane and averaged over the
waves, the Fq products (Fqm) of three walks:

  needed    what one lane needs on its own: a mixed addition per term, a full addition per rank
            left (empty ranks inside the slice included) and the small multiple;
  nested    the loops of rounds 1-9 as a wave executes them: at every rank step the longest inner
            loop of the 64 lanes, then the full addition, for as many rank steps as the lane that
            crosses most ranks; the multiple at the longest chain of the wave;
  walk      the lane-uniform walk (msm_walk.h): the longest slice of the wave in mixed additions,
            one full addition per flush round, the multiple at the longest chain.

A wave pays for an instruction when any of its lanes runs it, so every count is the wave's count
(all three are per lane of a full wave).  Costs: mixed addition 11, full addition 16, doubling 7
(bench/roofline_constants.json).  Identity and doubling branches, loads, the rank searches and the
snapshot stores are not counted.

    python3 tools/msm_walk_model.py --n 668 --bits 128 --c 7 --slots 1 2 4 16
"""
import argparse
import random

MADD, ADD, DBL = 11, 16, 7


def recode(k, c, W):
    half, out, carry = 1 << (c - 1), [], 0
    for w in range(W):
        v = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        if v > half:
            out.append(v - (1 << c))
            carry = 1
        else:
            out.append(v)
            carry = 0
    return out


def mul_cost(k, from_point):
    """[k] p MSB-first.  from_point: start at p (the walk); otherwise at the identity (rounds 1-9:
    a doubling and an addition per bit of k, the first of each on the identity still issued)."""
    if k == 0:
        return 0
    bits = k.bit_length()
    ones = bin(k).count("1")
    return (bits - 1) * DBL + (ones - 1) * ADD if from_point else bits * DBL + ones * ADD


def lane_plan(ranks, p0, p1, B):
    """ranks: rank of every sorted position.  Returns (terms per rank step, last rank) of the slice."""
    if p0 >= p1:
        return [], None
    r0, r1 = ranks[p0], ranks[p1 - 1]
    cnt = [0] * (r1 - r0 + 1)
    for e in range(p0, p1):
        cnt[ranks[e] - r0] += 1
    return cnt, r1


def walk_wave(plans, B, slots):
    """Replay of the lane-uniform walk on one wave: (steps, flush rounds)."""
    # per lane: the positions (relative to the slice) before which a rank is left, in order
    state = []
    for cnt, _ in plans:
        due, pos = [], 0
        for c in cnt[:-1]:
            pos += c
            due.append(pos)
        state.append({"len": sum(cnt), "due": due, "e": 0, "pend": 0, "next": 0})
    steps = rounds = 0
    while True:
        need = False
        for s in state:
            while s["e"] < s["len"] and s["next"] < len(s["due"]) and s["due"][s["next"]] <= s["e"]:
                if s["pend"] == slots:
                    need = True
                    break
                s["pend"] += 1
                s["next"] += 1
        if need:
            rounds += max(s["pend"] for s in state)
            for s in state:
                s["pend"] = 0
            continue
        if not any(s["e"] < s["len"] for s in state):
            break
        steps += 1
        for s in state:
            if s["e"] < s["len"]:
                s["e"] += 1
    rounds += max(s["pend"] for s in state)
    return steps, rounds


def model(n, bits, c, slots_list, n_msm, seed):
    rng = random.Random(seed)
    B = 1 << (c - 1)
    S = max(1, B // 8)
    W = (bits + c) // c
    plans = []  # lane order: (msm, window, segment)
    for _ in range(n_msm):
        digs = [recode(rng.getrandbits(bits - 1), c, W) for _ in range(n)]
        for w in range(W):
            ranks = sorted(B - abs(d[w]) for d in digs if d[w])
            total = len(ranks)
            for s in range(S):
                plans.append(lane_plan(ranks, total * s // S, total * (s + 1) // S, B))
    lanes = len(plans)
    need = nested = 0.0
    walk = {k: 0.0 for k in slots_list}
    parts = {k: [0.0, 0.0, 0.0] for k in slots_list}  # steps, flush rounds, tail Fqm (per wave, summed)
    waves = 0
    for w0 in range(0, lanes, 64):
        wave = plans[w0:w0 + 64]
        live = [(cnt, r1) for cnt, r1 in wave if cnt]
        for cnt, r1 in live:
            need += sum(cnt) * MADD + (len(cnt) - 1) * ADD + mul_cost(B - r1, True) + ADD
        if not live:
            continue
        waves += 1
        # rounds 1-9: rank step j costs the longest inner loop at step j, plus the full addition
        depth = max(len(cnt) for cnt, _ in live)
        inner = sum(max((cnt[j] for cnt, _ in live if j < len(cnt)), default=0) for j in range(depth))
        tail_old = max(mul_cost(B - r1 - 1, False) + (ADD if B - r1 - 1 else 0) for _, r1 in live)
        nested += 64 * (inner * MADD + depth * ADD + tail_old)
        tail_new = max(mul_cost(B - r1, True) for _, r1 in live) + ADD
        for k in slots_list:
            steps, rounds = walk_wave(live, B, k)
            walk[k] += 64 * (steps * MADD + rounds * ADD + tail_new)
            for j, v in enumerate((steps, rounds, tail_new)):
                parts[k][j] += v
    return (lanes, need / lanes, nested / lanes, {k: v / lanes for k, v in walk.items()},
            {k: [x / waves for x in v] for k, v in parts.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=668, help="terms per MSM (C3: 2 * 334 GLV halves)")
    ap.add_argument("--bits", type=int, default=128, help="scalar bits (GLV halves: 128)")
    ap.add_argument("--c", type=int, nargs="+", default=[7], help="window widths")
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 2, 4, 16], help="snapshot slots per lane")
    ap.add_argument("--msms", type=int, default=64, help="MSMs sampled")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    for c in a.c:
        lanes, need, nested, walk, parts = model(a.n, a.bits, c, a.slots, a.msms, a.seed)
        per_msm = lanes / a.msms
        print("n %d  bits %d  c %d: %d lanes per MSM" % (a.n, a.bits, c, per_msm))
        print("  needed            %7.0f Fqm/lane   %9.0f Fqm/MSM" % (need, need * per_msm))
        print("  nested loops      %7.0f Fqm/lane   %9.0f Fqm/MSM   %.2f x needed" %
              (nested, nested * per_msm, nested / need))
        for k in a.slots:
            print("  walk, %2d slot(s)  %7.0f Fqm/lane   %9.0f Fqm/MSM   %.2f x needed   %.2f x nested"
                  "   (per wave: %.1f steps, %.1f flush rounds, tail %.0f Fqm)" %
                  (k, walk[k], walk[k] * per_msm, walk[k] / need, walk[k] / nested, *parts[k]))


if __name__ == "__main__":
    main()
