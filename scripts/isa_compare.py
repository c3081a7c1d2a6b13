"""Device code of two trees, kernel by kernel (CPU only: hipcc cross-compiles).

    python scripts/isa_compare.py <csrc directory A> <csrc directory B> <file.hip> ... [--shrink <file.hip>] ... [--report <file>] [--title <text>] [--labels <A> <B>]

Each file is compiled on both sides with hipcc <build.FLAGS + build.EXTRA_FLAGS[file]> --cuda-device-only -cuid=isa_compare -S -o - (the fixed -cuid keeps the
per-file marker object's name independent of the path).  Lines whose first non-blank characters are `.file` or `.ident` and lines that start with `;` are dropped,
and the text is split per kernel symbol.  Per kernel:
    equal     the same text once the symbol's own name and the function number in the labels `.LBB<n>_` / `.Lfunc_end<n>` are replaced by placeholders
    renamed   the same opcode histogram and the same .vgpr_count, .sgpr_count, .vgpr_spill_count, .private_segment_fixed_size, .group_segment_fixed_size
    differs   the histogram differences by class (v_mfma*, ds_*, global_* / buffer_*, s_waitcnt, s_barrier, other VALU, other SALU, other) and the metadata differences
Checked for every kernel of B that A has too: no spill and no private segment, .vgpr_count and .group_segment_fixed_size not above A's, and the counts of the
v_mfma* / ds_* / global_* / buffer_* / s_waitcnt / s_barrier classes equal to A's (files named with --shrink: not above A's).  Exit status 1 when a check fails."""
import collections
import hashlib
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
CLASSES = ("v_mfma*", "ds_*", "global_*/buffer_*", "s_waitcnt", "s_barrier", "other VALU", "other SALU", "other")
PINNED = CLASSES[:5]


def _build():
    spec = importlib.util.spec_from_file_location("_e2eft_build", os.path.join(ROOT, "diffusion-e2e-ft_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, csrc, name):
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA_FLAGS.get(name, []) + ["--cuda-device-only", "-cuid=isa_compare", "-S", "-o", "-", os.path.join(csrc, name)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (os.path.join(csrc, name), r.stderr))
    return [ln for ln in r.stdout.split("\n") if not ln.lstrip().startswith((".file", ".ident")) and not ln.startswith(";")]


def klass(op):
    if op.startswith("v_mfma"):
        return CLASSES[0]
    if op.startswith("ds_"):
        return CLASSES[1]
    if op.startswith(("global_", "buffer_")):
        return CLASSES[2]
    if op in ("s_waitcnt", "s_barrier"):
        return op
    if op.startswith("v_"):
        return CLASSES[5]
    if op.startswith("s_"):
        return CLASSES[6]
    return CLASSES[7]


def kernels(lines):
    """{symbol: {"text": normalised body, "ops": Counter of opcodes, "meta": {key: int}, "lines": n}}"""
    out, meta = {}, {}
    entry = None
    for ln in lines:                                   # the amdhsa.kernels list of the metadata note: one `  - ` entry per kernel
        if ln.startswith("  - "):
            entry = {}
            ln = "    " + ln[4:]
        m = re.match(r"\s+(\.[a-z_]+):\s+(\S+)\s*$", ln)
        if entry is not None and m:
            if m.group(1) == ".name":
                meta[m.group(2)] = entry
            elif m.group(1) in META:
                entry[m.group(1)] = int(m.group(2))
    i = 0
    while i < len(lines):
        m = re.match(r"\s+\.amdhsa_kernel\s+(\S+)", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        start = max(j for j in range(i) if lines[j].startswith(sym + ":"))
        end = next(j for j in range(i, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        body = lines[start:end + 1]
        text = "\n".join(re.sub(r"\.Lfunc_end\d+", ".Lfunc_end<f>", re.sub(r"\.LBB\d+_", ".LBB<f>_", ln.replace(sym, "<kernel>"))) for ln in body)
        ops = collections.Counter()
        for ln in lines[start + 1:i]:
            tok = ln.split()
            if ln.startswith("\t") and tok and not tok[0].startswith((".", ";")) and not tok[0].endswith(":"):
                ops[tok[0]] += 1
        out[sym] = {"text": text, "ops": ops, "meta": meta.get(sym, {}), "lines": len(body)}
        i = end + 1
    return out


def compare(dir_a, dir_b, files, shrink=(), title=None, labels=None):
    build = _build()
    lines, bad = [], 0
    ver = subprocess.run([build._hipcc(), "--version"], capture_output=True, text=True).stdout.split("\n")[0]
    lines += [title or "Device code of A against B, kernel by kernel", "",
              "A: %s" % (labels or (dir_a, dir_b))[0], "B: %s" % (labels or (dir_a, dir_b))[1],
              "Method (scripts/isa_compare.py): hipcc <build.FLAGS + build.EXTRA_FLAGS[file]> --cuda-device-only -cuid=isa_compare -S; `.file` / `.ident` / `;` lines dropped; per kernel",
              "symbol: equal = same text with the symbol's name and the function number of its labels replaced; renamed = same opcode histogram and register / LDS / scratch",
              "metadata; otherwise the differences by class.  Compiler: %s, %s." % (ver, " ".join(f for f in build.FLAGS if f.startswith("--offload-arch"))), ""]
    tally = collections.Counter()
    for name in files:
        ka, kb = kernels(assembly(build, dir_a, name)), kernels(assembly(build, dir_b, name))
        lines.append("%s%s" % (name, "  (classes may only shrink)" if name in shrink else ""))
        for sym in sorted(set(ka) | set(kb)):
            if sym not in ka or sym not in kb:
                lines.append("  %-90s only in %s" % (sym, "A" if sym in ka else "B"))
                tally["one side"] += 1
                continue
            a, b = ka[sym], kb[sym]
            ca, cb = collections.Counter(), collections.Counter()
            for op, n in a["ops"].items():
                ca[klass(op)] += n
            for op, n in b["ops"].items():
                cb[klass(op)] += n
            dmeta = [(k, a["meta"].get(k), b["meta"].get(k)) for k in META if a["meta"].get(k) != b["meta"].get(k)]
            if a["text"] == b["text"]:
                verdict = "equal"
            elif a["ops"] == b["ops"] and not dmeta:
                verdict = "renamed"
            else:
                verdict = "differs"
            tally[verdict] += 1
            mb = b["meta"]
            regs = "vgpr %s sgpr %s spill %s scratch %s lds %s" % tuple(mb.get(k, "?") for k in META)
            lines.append("  %-90s %5d / %5d lines  %s %s  %-7s  %s" % (sym, a["lines"], b["lines"], hashlib.sha256(a["text"].encode()).hexdigest()[:12],
                                                                      hashlib.sha256(b["text"].encode()).hexdigest()[:12], verdict, regs))
            if verdict == "differs":
                for k, x, y in dmeta:
                    lines.append("      %s: %s -> %s" % (k, x, y))
                for c in CLASSES:
                    ops = sorted(op for op in set(a["ops"]) | set(b["ops"]) if klass(op) == c and a["ops"][op] != b["ops"][op])
                    if ops:
                        lines.append("      %-18s %5d -> %5d   %s" % (c, ca[c], cb[c], ", ".join("%s %+d" % (op, b["ops"][op] - a["ops"][op]) for op in ops)))
            fails = []
            if mb.get(".vgpr_spill_count", 0) or mb.get(".private_segment_fixed_size", 0):
                fails.append("spill / scratch")
            for k in (".vgpr_count", ".group_segment_fixed_size"):
                if mb.get(k, 0) > a["meta"].get(k, 0):
                    fails.append("%s above A's" % k)
            for c in PINNED:
                if cb[c] > ca[c] or (cb[c] != ca[c] and name not in shrink):
                    fails.append("%s count %d -> %d" % (c, ca[c], cb[c]))
            if fails:
                bad += 1
                lines.append("      CHECK FAILED: " + "; ".join(fails))
        lines.append("")
    lines.append("kernels: " + ", ".join("%d %s" % (n, k) for k, n in sorted(tally.items())) + "; checks failed: %d" % bad)
    return "\n".join(lines) + "\n", bad


if __name__ == "__main__":
    args, shrink, report, title, labels = [], [], None, None, None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--shrink":
            shrink.append(next(it))
        elif a == "--report":
            report = next(it)
        elif a == "--title":
            title = next(it)
        elif a == "--labels":
            labels = (next(it), next(it))
        else:
            args.append(a)
    if len(args) < 3:
        sys.exit(__doc__)
    text, bad = compare(args[0], args[1], args[2:], shrink, title, labels)
    sys.stdout.write(text)
    if report:
        with open(report, "w") as f:
            f.write(text)
    sys.exit(1 if bad else 0)
