#!/usr/bin/env python3
"""Static instruction budget of k_screen_mx_cull<NCT>, counted from the compiler's assembly (no GPU).

    hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -Iinclude -Imultimoda-rs_amd/csrc \\
          --cuda-device-only -S multimoda-rs_amd/csrc/mm_kernels.hip -o mm_kernels.s
    python tools/count_cull_isa.py mm_kernels.s --nct 17 --nrt 17 --tiles 60 --group 8 --early 0.8

The kernel's candidate loop carries section marks, comment lines `; mxc:<name>:<trips>` that emit no instruction.  Every
instruction line after a mark belongs to that section, in the TEXT order of the assembly (the compiler may place a block
away from its source position: a few instructions land in a neighbouring section; the sums are not affected).  <trips> says
how often the section runs per candidate:

    1        once                       nrt      once per row tile            half     once per two row tiles
    rows2    once per row tile that has tiles left in phase 2 (--rows2, default nrt: the upper bound)
    pairs64  once per 64 tile pairs     tiles    once per computed tile (summed over the copies, divided by their number)
    group    once per group of --group candidates (1 / G per candidate)      ghalf    `half`, per group
    gnrt     `nrt`, per group           lead     once per leader (a group's first candidate; the value floor's sections: flr_tr
             and flr_tc_row, Tr_I / Tc_J of the group's phase-1 mask, and flr_lead, the leader's floor L)
    fgroup   once per group that has followers (1 / G per candidate, none at G = 1)     fgnrt    `nrt`, per such group
    fghalf   `half`, per such group
    fol      once per follower of a group ((G - 1) / G per candidate)        frows    `nrt`, per follower
    lrows    `nrt`, per leader (a group's first candidate: 1 / G per candidate)
    early    once per follower that leaves after phase 1 on the group test (--early: their share of the followers, from
             tools/model_cull_tiles.py --group G)
    late     once per candidate that does not leave early (1 - early (G - 1) / G)
    0        not in the candidate loop

The prologue in front of the candidate loop is charged per candidate too, from --run-items and --item-cands:

    item     once per work item (pro_item: the item's WorkItem, its candidates' cos / sin, the barriers):
             1 / --item-cands per candidate
    run      once per run of --run-items work items that one workgroup executes (pro_run: the pair's row fragments, target
             points, norms and circles, staged at the run's first item): 1 / (--run-items x --item-cands) per candidate.  A
             workgroup per item is --run-items 1.  The section's loops (a tile's circle is two serial loops over 32 points,
             mx_stage_rows one over the row tiles) count once: the static figure is a floor of what a run executes

Pairs (--pair, default on, the set-bit variant at G >= 4): a group's followers run two at a time, P = (G - 2) // 2 pairs a group,
so 2 P / G of the candidates are paired, (G - 1 - 2 P) / G are single followers:

    pair     once per pair (P / G per candidate)        prows    `nrt`, per pair        ptiles   once per tile of a pair (a section
             named `tile2` is the paired tile body: the MFMAs behind a tloop2 / tile2 mark count to it)
    xcand    once per candidate that is not a pair's second (1 - P / G)       single   once per candidate outside a pair
    sfol     once per single follower                   sfrows   `nrt`, per single follower (what frows counts with --pair 0)
    searly   once per single follower that leaves early               pearly   once per pair whose X (or whose Y) leaves early
    ylate    once per pair's second follower that does not leave early
    tails    once per computed tile of the LAST column tile, which has a register of its own and a body (`tilet`, paired
             `tile2t`: ptails) behind the loop over the others; --tail is its share of the computed tiles (default 1 / NCT)
    tiles    ... of the candidates outside a pair (their phase-2 tiles, few, are charged to the pairs' loop at its rate)

and a section named `tile` is a computed tile's own body (its copies are averaged; every v_mfma counts to it).  A section
ends at the next mark or at an unconditional branch; instructions between such a branch and the next mark are listed as
`unmarked` and not charged.  Instructions are classified by the
mnemonic's prefix only: v_mfma, other v_, s_, ds_, global_/flat_/buffer_.  The estimate counts every instruction of a section
as executed, also those a branch skips (rare paths are charged in full), and leaves out the `unmarked` blocks, some of which
the compiler moved out of the candidate loop's text (register-vector copies at a loop exit, for instance): it is a count for
comparing two builds of the kernel section by section, neither a bound nor a time.
"""
import argparse
import re
import sys
from collections import OrderedDict

CLASSES = ("mfma", "valu", "salu", "lds", "vmem", "other")


def classify(mn):
    if mn.startswith("v_mfma"):
        return "mfma"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    return "other"


def kernels(text):
    """{NCT: (body lines, info lines)} of every k_screen_mx_cull<NCT> in the assembly."""
    out = {}
    lines = text.splitlines()
    i = 0
    head = re.compile(r"^(_Z\w*k_screen_mx_cullILi(\d+)E\w*):")
    while i < len(lines):
        m = head.match(lines[i])
        if not m:
            i += 1
            continue
        nct = int(m.group(2))
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        k = j
        while k < len(lines) and k < j + 400 and not head.match(lines[k]) and not lines[k].startswith("; Occupancy"):
            k += 1
        k = min(k + 1, len(lines))
        out[nct] = (lines[i + 1:j], lines[j:k])
        i = k
    return out


def info(lines, key):
    for ln in lines:
        m = re.match(r"^;\s*" + re.escape(key) + r":\s*(\d+)", ln)
        if m:
            return int(m.group(1))
    return None


def sections(body):
    """OrderedDict name -> {"trips": str, "entries": int, class: count}; the code before the first mark is `item`."""
    secs = OrderedDict()

    def sec(name, trips):
        if name not in secs:
            secs[name] = dict(trips=trips, entries=0, **{c: 0 for c in CLASSES})
        return secs[name]

    cur = sec("item", "0")
    for ln in body:
        m = re.search(r";\s*mxc:([A-Za-z0-9_]+)(?::([A-Za-z0-9_]+))?", ln)
        if m:
            cur = sec(m.group(1), m.group(2) or ("tile" if m.group(1) == "tile" else "1"))
            cur["entries"] += 1
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]*)\b", ln)
        if not m or ln.lstrip().startswith((".", ";")):
            continue
        mn, cl = m.group(1), classify(m.group(1))
        if cl == "mfma":                                             # (the scheduler may lift a tile's MFMAs above its mark)
            if cur is secs.get("tilet") or cur is secs.get("tile2t"):
                cur[cl] += 1                                             # (the last column tile's body, reached by name)
            else:
                paired = cur is secs.get("tloop2") or cur is secs.get("tile2") or cur is secs.get("p1p_row")
                (sec("tile2", "ptiles") if paired else sec("tile", "tile"))[cl] += 1
        else:
            cur[cl] += 1
        if mn in ("s_branch", "s_endpgm") or mn.startswith("s_setpc"):
            cur = sec("unmarked", "0")                               # no fall-through: what follows is another block
    return secs


def report(nct, body, inf, nrt, tiles, rows2, out, group=1, early=0.0, pair=True, tail=None, run_items=1.0, item_cands=32.0,
           unmarked="0"):
    secs = sections(body)
    if "unmarked" in secs:
        secs["unmarked"]["trips"] = unmarked
    copies = max(1, secs["tile"]["entries"]) if "tile" in secs else 1
    fol = (group - 1.0) / group
    fgroup = 1.0 / group if group > 1 else 0.0
    tcopies = max(1, secs["tilet"]["entries"]) if "tilet" in secs else 1
    tail = (1.0 / nct if tail is None else tail) if "tilet" in secs else 0.0     # share of the computed tiles in the last column tile
    npair = max(0, (group - 2) // 2) if pair and "tile2" in secs else 0      # pairs per group: followers 1 .. 2 P
    pshare, sfol = 2.0 * npair / group, (group - 1.0 - 2 * npair) / group
    trips = {"0": 0.0, "1": 1.0, "item": 1.0 / item_cands, "run": 1.0 / (run_items * item_cands), "nrt": float(nrt), "half": float((nrt + 1) // 2), "rows2": float(rows2),
             "pairs64": float((nrt * nct + 63) // 64), "tiles": tiles * (1.0 - pshare) * (1.0 - tail) / copies,
             "tile": tiles * (1.0 - pshare) * (1.0 - tail) / copies, "tails": tiles * (1.0 - pshare) * tail / tcopies,
             "ptiles": tiles * pshare * (1.0 - tail) / 2, "ptails": tiles * pshare * tail / 2, "pair": pshare / 2, "prows": nrt * pshare / 2, "xcand": 1.0 - pshare / 2,
             "single": 1.0 - pshare, "sfol": sfol, "sfrows": nrt * sfol, "searly": early * sfol, "pearly": early * pshare / 2,
             "ylate": (1.0 - early) * pshare / 2,
             "group": 1.0 / group, "ghalf": float((nrt + 1) // 2) / group, "gnrt": float(nrt) / group, "lead": 1.0 / group,
             "fgroup": fgroup, "fgnrt": nrt * fgroup, "fghalf": float((nrt + 1) // 2) * fgroup,
             "fol": fol, "frows": nrt * sfol, "lrows": nrt * (1.0 - fol), "early": early * fol, "late": 1.0 - early * fol}
    out.write("k_screen_mx_cull<%d>: VGPRs %s, AGPRs %s, scratch %s bytes/lane, occupancy %s waves/SIMD\n" % (
        nct, info(inf, "NumVgprs"), info(inf, "NumAgprs"), info(inf, "ScratchSize"), info(inf, "Occupancy")))
    out.write("  trip counts: nrt %d, NCT %d, tiles/candidate %g, phase-2 row tiles %g, candidates/group %d, early share of the followers %g; tile bodies in the code: %d\n" % (
        nrt, nct, tiles, rows2, group, early, copies))
    out.write("  prologue: %g candidates per work item, %g work items per run\n" % (item_cands, run_items))
    out.write("  %-10s %-8s %6s %6s %6s %6s %6s %6s %7s %9s\n" % ("section", "trips", "mfma", "valu", "salu", "lds", "vmem",
                                                                  "other", "static", "executed"))
    tot_tile = tot_rest = tot_pro = 0.0
    by_class = {c: 0.0 for c in CLASSES}                                 # executed per candidate, the candidate loop's sections
    for name, s in secs.items():
        static = sum(s[c] for c in CLASSES)
        if s["trips"] not in trips:
            raise SystemExit("unknown trip count %r in mark %r" % (s["trips"], name))
        ex = static * trips[s["trips"]]
        if s["trips"] in ("item", "run"):
            tot_pro += ex
        elif name in ("tile", "tile2", "tilet", "tile2t"):
            tot_tile += ex
        else:
            tot_rest += ex
        if s["trips"] not in ("item", "run"):
            for c in CLASSES:
                by_class[c] += s[c] * trips[s["trips"]]
        out.write(("  %-10s %-8s %6d %6d %6d %6d %6d %6d %7d %9.1f\n" if s["trips"] in ("item", "run") else
                   "  %-10s %-8s %6d %6d %6d %6d %6d %6d %7d %9.0f\n") % (name, s["trips"], s["mfma"], s["valu"], s["salu"], s["lds"],
                                                                       s["vmem"], s["other"], static, ex))
    if "tile" in secs:
        out.write("  a computed tile's body: %.1f instructions\n" % (sum(secs["tile"][c] for c in CLASSES) / copies))
    if "tile2" in secs:
        out.write("  a paired tile's body (two candidates): %.1f instructions; pairs per group %d\n" % (sum(secs["tile2"][c] for c in CLASSES), npair))
    out.write("  executed per candidate by class: " + ", ".join("%s %.0f" % (c, by_class[c]) for c in CLASSES if by_class[c]) + "\n")
    out.write("  executed per candidate: tiles %.0f, everything else %.0f" % (tot_tile, tot_rest))
    out.write("; the prologue %.1f (static, its loops counted once)\n\n" % tot_pro if tot_pro else "\n\n")
    return tot_tile, tot_rest


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", help="assembly of mm_kernels.hip (hipcc ... -S --cuda-device-only)")
    ap.add_argument("--nct", type=int, default=17, help="column tiles: which k_screen_mx_cull<NCT> (0: all)")
    ap.add_argument("--nrt", type=int, default=17, help="row tiles of the pair")
    ap.add_argument("--tiles", type=float, default=60, help="tiles computed per candidate")
    ap.add_argument("--rows2", type=float, default=None, help="row tiles with tiles left in phase 2 (default: nrt)")
    ap.add_argument("--group", type=int, default=1, help="candidates per group: the sections marked group / ghalf run once per group")
    ap.add_argument("--early", type=float, default=0.0, help="share of a group's followers that leave after phase 1 (sections marked early / late)")
    ap.add_argument("--tail", type=float, default=None, help="share of the computed tiles that are the last column tile's (default 1 / NCT)")
    ap.add_argument("--pair", type=int, default=1, help="0: the pair switch off (every follower runs alone)")
    ap.add_argument("--run-items", type=float, default=1.0, help="work items per run (sections marked run: once per run); 1: a workgroup per item")
    ap.add_argument("--unmarked", choices=("0", "run"), default="0",
                    help="run: charge the unmarked blocks once per run too -- most of them are blocks of the staging that lie behind a "
                         "branch (the circles' loops, the row fragments); with the marked part, the two ends of the prologue's static cost")
    ap.add_argument("--item-cands", type=float, default=32.0, help="candidates per work item (sections marked item and run)")
    a = ap.parse_args(argv)
    if a.group < 1:
        raise SystemExit("--group must be at least 1")
    if not 0.0 <= a.early <= 1.0:
        raise SystemExit("--early is a share, 0 .. 1")
    if a.run_items < 1 or a.item_cands < 1:
        raise SystemExit("--run-items and --item-cands must be at least 1")
    with open(a.asm) as f:
        ks = kernels(f.read())
    if not ks:
        raise SystemExit("no k_screen_mx_cull in " + a.asm)
    for nct in sorted(ks):
        if a.nct and nct != a.nct:
            continue
        body, inf = ks[nct]
        report(nct, body, inf, a.nrt, a.tiles, a.nrt if a.rows2 is None else a.rows2, sys.stdout, a.group, a.early, a.pair != 0, a.tail,
               a.run_items, a.item_cands, a.unmarked)


if __name__ == "__main__":
    main()
