#!/usr/bin/env python3
"""Static ISA census of one kernel in a `hipcc --cuda-device-only -S` listing (dev tool).

    python tools/isa/census.py /tmp/pk.s 'packet_direct_kernelILi1ELi0ELb0ELb0ELi1E' [--blocks]
    python tools/isa/census.py /tmp/pk.s packet_direct_kernel --folded
    python tools/isa/census.py /tmp/pk.s packet_direct_kernel --uniform

Counts the instructions of the kernel by class (FP64 / FP32 / int VALU, v_cndmask, v_mov,
v_cmp, SALU, LDS, global, branches), and with --blocks prints every basic block with its size
and class counts, so that the blocks of the hot path can be attributed to source phases.

--folded checks EVERY kernel of the listing whose name contains the pattern for basic blocks
that hold both a shared-reciprocal division core and full IEEE divisions by the same divisor
(unit() / light_dir() of rt_device.hpp with the fallback branch if-converted into the core:
every lane then pays for both).  Such a block has ≥ 4 v_rcp_f64 and ≥ 3 v_div_fixup_f64, but so
have blocks of four or more honest divisions (light_dir's fallback, the tonemap), so the
signature is the operand: the core takes v_rcp_f64 of the divisor itself, a full division takes
it of the v_div_scale_f64 result and names the divisor only in its v_div_fixup_f64.  A block
where a v_rcp_f64 source is also, unmodified, the denominator of ≥ 3 v_div_fixup_f64 is
reported.  Prints one line per such block and exits 1 when there is any.
--shared N lowers the number of divisions that must share the core's divisor (default 3:
unit() and light_dir()); --shared 1 also reports a single-division core (plane_t_core,
sphere_roots_core, reinhard_byte) computed in one block with its full-division fallback.

--uniform lists, for EVERY kernel whose name contains the pattern, the VALU arithmetic and
conversion instructions all of whose sources are wave-uniform (SGPRs, literals, inline
constants; propagated through v_mov from such a source and through the listed instructions
themselves inside a basic block): per-lane work for one value per wave, which belongs on the
host, once per frame, or behind a wave-uniform branch (tests/test_isa_uniform.py).

A basic block starts at a label (.LBBn_m) or at a fall-through block comment (; %bb.n)."""
import re
import sys
from collections import Counter, OrderedDict

FOLD_MIN_FIXUP = 3  # full divisions sharing the core's divisor: unit() has three


def classify(op):
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith(("v_mov", "v_readlane", "v_readfirstlane", "v_writelane")):
        return "v_mov/lane"
    if op.startswith(("v_cmp", "v_cmpx")):
        return "v_cmp_f64" if "f64" in op else "v_cmp_other"
    if op.startswith("v_"):
        if "f64" in op:
            if any(k in op for k in ("rcp", "rsq", "sqrt", "div_scale", "div_fmas", "div_fixup",
                                     "ldexp", "frexp", "trig", "class")):
                return "v_f64_special"
            return "v_f64_arith"
        if "f32" in op or "f16" in op:
            return "v_f32"
        if "dpp" in op:
            return "v_dpp"
        return "v_int/bit"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith("s_waitcnt") or op.startswith("s_nop") or op.startswith("s_barrier"):
        return "s_wait/nop"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem:" + ("scratch" if op.startswith("scratch") or "buffer" in op else "global")
    return "other"


_BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; (%bb\.\d+):)")


def kernels(lines, name):
    """{mangled kernel name: OrderedDict(block -> [instruction lines])} of every kernel whose
    name contains `name`."""
    out = OrderedDict()
    i = 0
    while i < len(lines):
        l = lines[i]
        if l.startswith("_Z") and name in l and (l.rstrip().endswith(":") or ": ;" in l):
            kname = l.split(":")[0]
            end = next(j for j in range(i + 1, len(lines)) if lines[j].startswith(".Lfunc_end"))
            blocks = OrderedDict()
            cur = "entry"
            blocks[cur] = []
            for b in lines[i + 1:end]:
                s = b.strip()
                m = _BLOCK.match(s)
                if m:
                    cur = m.group(1) or m.group(2)
                    blocks[cur] = []
                    continue
                if not s or s.startswith(";") or s.startswith("."):
                    continue
                blocks[cur].append(s.split(";")[0].strip())
            out[kname] = blocks
            i = end
        i += 1
    return out


_REG = re.compile(r"([vs])\[(\d+):(\d+)\]|([vs])(\d+)")


def _regs(operand):
    """(file, first, last) of a register operand such as -v[6:7], |v[0:1]| or v3; else None."""
    m = _REG.search(operand)
    if not m:
        return None
    if m.group(1):
        return m.group(1), int(m.group(2)), int(m.group(3))
    return m.group(4), int(m.group(5)), int(m.group(5))


def _operands(line):
    parts = line.split(None, 1)
    return [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []


def folded_blocks(blocks, min_shared=None):
    """[(block, size, #v_rcp_f64, #v_div_fixup_f64, #shared)] of the blocks where a v_rcp_f64
    takes the very divisor of `shared` ≥ min_shared (default FOLD_MIN_FIXUP) v_div_fixup_f64
    (no write in between)."""
    if min_shared is None:
        min_shared = FOLD_MIN_FIXUP
    hits = []
    for b, ins in blocks.items():
        rcps = [i for i, l in enumerate(ins) if l.startswith("v_rcp_f64")]
        fixs = [i for i, l in enumerate(ins) if l.startswith("v_div_fixup_f64")]
        best = 0
        for i in rcps:
            src = _regs(_operands(ins[i])[1])
            if src is None:
                continue
            shared = 0
            for j in fixs:
                if j < i or _regs(_operands(ins[j])[2]) != src:
                    continue
                written = False
                for k in range(i + 1, j):
                    ops = _operands(ins[k])
                    d = _regs(ops[0]) if ops and ins[k].startswith("v_") else None
                    if d and d[0] == src[0] and d[1] <= src[2] and src[1] <= d[2]:
                        written = True
                        break
                shared += not written
            best = max(best, shared)
        if best >= min_shared:
            hits.append((b, len(ins), len(rcps), len(fixs), best))
    return hits


_MODIFIER_LIST = re.compile(r"\s+\w+:\[[^\]]*\]")
_CONST = re.compile(r"^(?:0x[0-9a-f]+|[0-9]+(?:\.[0-9]+)?(?:e[-+]?[0-9]+)?|m0|ttmp\d+|ttmp\[\d+:\d+\]|"
                    r"src_\w+)$")
_UNIFORM_CLASSES = ("v_f64_arith", "v_f64_special", "v_f32", "v_int/bit")
# a lane mask (carry, select, scale flag) or the lane number is an input the operands do not show
_LANE_INPUT = ("addc", "subb", "cndmask", "div_fmas", "mbcnt", "dpp", "sdwa", "permlane", "swap")
_TWO_DESTS = ("_co_", "div_scale", "mad_u64_u32", "mad_i64_i32")


def _strip(operand):
    """An operand without its sign / abs modifiers and trailing instruction modifiers."""
    o = operand.split()[0] if operand.split() else ""
    o = re.sub(r"^(?:neg|abs)\((.*)\)$", r"\1", o)
    return o.lstrip("-").strip("|")


def uniform_valu(blocks):
    """[(block, instruction)] of the VALU arithmetic and conversion instructions all of whose
    sources are wave-uniform: SGPRs, literals, inline constants, and VGPRs that hold such a
    value — written, earlier in the same basic block and not since, by a v_mov from a uniform
    source or by an instruction reported here.  Every lane of the wave computes the same value:
    a candidate for the host (once per frame) or for a wave-uniform branch.  Instructions that
    read a lane mask or the lane number besides their operands are never reported."""
    hits = []
    for b, ins in blocks.items():
        uni = set()  # VGPR numbers holding a wave-uniform value at this point of the block
        for l in ins:
            op = l.split()[0]
            ops = _operands(_MODIFIER_LIST.sub("", l))
            if not op.startswith("v_"):
                # loads write their first operand; stores only read it: forgetting is safe
                d = _regs(ops[0]) if ops else None
                if d and d[0] == "v":
                    uni.difference_update(range(d[1], d[2] + 1))
                continue
            ndst = 2 if any(k in op for k in _TWO_DESTS) else 1
            srcs = [_strip(o) for o in ops[ndst:]]

            def is_uniform(o):
                if _CONST.match(o.lower()):
                    return True
                r = _regs(o)
                if r is None or o.lower().startswith(("vcc", "exec")):
                    return False
                return r[0] == "s" or all(k in uni for k in range(r[1], r[2] + 1))

            cls = classify(op)
            uniform = bool(srcs) and not any(k in op for k in _LANE_INPUT) and \
                all(is_uniform(o) for o in srcs)
            dst = _regs(ops[0]) if ops else None
            if dst and dst[0] == "v":
                regs = range(dst[1], dst[2] + 1)
                if uniform and (op.startswith("v_mov_b") or cls in _UNIFORM_CLASSES):
                    uni.update(regs)
                else:
                    uni.difference_update(regs)
            if uniform and cls in _UNIFORM_CLASSES:
                hits.append((b, l))
    return hits


def main():
    path, name = sys.argv[1], sys.argv[2]
    found = kernels(open(path).read().splitlines(), name)
    if not found:
        sys.exit(f"no kernel matching {name!r} in {path}")
    if "--uniform" in sys.argv:
        for kname, blocks in found.items():
            hits = uniform_valu(blocks)
            print(f"{kname}: {len(hits)} VALU arithmetic / conversion instructions with "
                  f"wave-uniform sources only")
            for b, l in hits:
                print(f"  {b:14s} {l}")
        return
    if "--folded" in sys.argv:
        bad = 0
        shared = int(sys.argv[sys.argv.index("--shared") + 1]) if "--shared" in sys.argv else None
        for kname, blocks in found.items():
            hits = folded_blocks(blocks, shared)
            bad += len(hits)
            print(f"{kname}: {len(hits)} folded core+division blocks in {len(blocks)} blocks")
            for b, n, rcp, fix, shared in hits:
                print(f"  {b:14s} {n:5d} instructions  v_rcp_f64={rcp} v_div_fixup_f64={fix} "
                      f"(core divisor shared by {shared})")
        sys.exit(1 if bad else 0)
    kname, blocks = next(iter(found.items()))
    total = Counter(classify(o.split()[0]) for b in blocks.values() for o in b)
    n = sum(total.values())
    print(f"{name}: {n} instructions in {len(blocks)} blocks")
    for k, v in total.most_common():
        print(f"  {k:16s} {v:6d}")
    if "--blocks" in sys.argv:
        for b, ops in blocks.items():
            c = Counter(classify(o.split()[0]) for o in ops)
            print(f"{b:14s} {len(ops):5d}  " + " ".join(f"{k}={v}" for k, v in c.most_common(6)))


if __name__ == "__main__":
    main()
