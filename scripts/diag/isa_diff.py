#!/usr/bin/env python3
"""Compare the device code of two builds of a translation unit, kernel by kernel.

Both inputs are assembly files of the same source at two commits, device side only:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-strict-aliasing \\
          --cuda-device-only -S index_search.hip -o X.s

A unit that was split (or several units: index_search.hip, index_store.hip,
index_shardset.hip) is compared as the concatenation of its units' assembly files.

For every kernel symbol the text between its label and its end label is taken, comment, debug
and unwind lines are dropped and the local label numbers are renumbered in order of appearance,
so two bodies compare equal exactly when they hold the same instructions in the same order.
The kernel's resource notes (registers, scratch, LDS, occupancy) come from its descriptor and
the compiler's kernel-info comments.

Output (JSON lines): a head line with the counts, then one line per kernel that differs or
exists on one side only, parent against result. `--must-match REGEX` (repeatable) names kernels
that have to be identical; the exit status is 1 if one of them differs, if a kernel's scratch
grows from 0 or if its occupancy drops.

Kernels are paired by their demangled names. `--rename 'REGEX=REPLACEMENT'` (repeatable, applied
in order, `\\1` for a group) rewrites the parent's demangled names before pairing, so that a
kernel that changed its name or its template arguments is compared with its predecessor and the
scratch and occupancy conditions hold for it too; without it both sides are reported as "only
in" and the tool fails (a name the demangler cannot read stays mangled; its rename is written
over the mangled form):

    --rename 'sample_kernel_i8<(\\d+), (\\w+)>=sample_kernel_q<\\1, \\2, ragmi::Copy8>'

    python scripts/diag/isa_diff.py parent.s result.s [--must-match 'scan_kernel'] \\
           [--rename 'OLD=NEW'] > record.jsonl
"""
from __future__ import annotations

import argparse
import json
import re
import subprocess
import sys

_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_LOCAL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
_SKIP = re.compile(r"^\s*(;|\.loc\b|\.file\b|\.cfi_|\.p2align|$)")
# resource notes: descriptor fields and kernel-info comments
_NOTES = {
    "vgpr": re.compile(r";\s*NumVgprs:\s*(\d+)"),
    "agpr": re.compile(r";\s*NumAgprs:\s*(\d+)"),
    "sgpr": re.compile(r";\s*TotalNumSgprs:\s*(\d+)"),
    "scratch": re.compile(r";\s*ScratchSize:\s*(\d+)"),
    "lds": re.compile(r";\s*LDSByteSize:\s*(\d+)"),
    "occupancy": re.compile(r";\s*Occupancy:\s*(\d+)"),
}


def _normalise(lines: list[str]) -> list[str]:
    names: dict[str, str] = {}

    def local(m: re.Match) -> str:
        return names.setdefault(m.group(0), f".L{len(names)}")

    out = []
    for ln in lines:
        if _SKIP.match(ln):
            continue
        ln = ln.split(";", 1)[0].rstrip()     # trailing comments
        if ln:
            out.append(_LOCAL.sub(local, ln))
    return out


def kernels(path: str) -> dict[str, dict]:
    """symbol -> {"body": normalised lines, notes...} for every kernel of an assembly file."""
    text = open(path).read().split("\n")
    kernel_syms = set()
    for ln in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            kernel_syms.add(m.group(1))
    res: dict[str, dict] = {}
    i, n = 0, len(text)
    while i < n:
        m = _LABEL.match(text[i])
        if not (m and m.group(1) in kernel_syms and m.group(1) not in res):
            i += 1
            continue
        sym = m.group(1)
        j = i + 1
        while j < n and not text[j].startswith(".Lfunc_end"):
            j += 1
        # (the kernel's own symbol, in its descriptor and section lines, is not code: a renamed
        # kernel with the same instructions compares equal)
        entry: dict = {"body": [ln.replace(sym, "<self>") for ln in _normalise(text[i + 1:j])]}
        # the kernel-info comments follow the end label, up to the next section or label
        k = j + 1
        while k < n and not _LABEL.match(text[k]) and not text[k].lstrip().startswith(".amdhsa_kernel"):
            for key, rx in _NOTES.items():
                mm = rx.search(text[k])
                if mm and key not in entry:
                    entry[key] = int(mm.group(1))
            k += 1
        res[sym] = entry
        i = j + 1
    return res


def demangle(syms: list[str]) -> dict[str, str]:
    try:
        out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True,
                             check=True).stdout.split("\n")
        return dict(zip(syms, out))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("result")
    ap.add_argument("--must-match", action="append", default=[],
                    help="regex over the symbol or its demangled name: must be identical")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT",
                    help="rewrite the parent's demangled names before pairing")
    a = ap.parse_args()
    renames = []
    for spec in a.rename:
        rx, eq, to = spec.partition("=")
        if not eq:
            ap.error(f"--rename {spec!r}: expected REGEX=REPLACEMENT")
        renames.append((re.compile(rx), to))

    def renamed(name: str) -> str:
        for rx, to in renames:
            name = rx.sub(to, name)
        return name

    old_syms, new_syms = kernels(a.parent), kernels(a.result)
    dem = demangle(sorted(set(old_syms) | set(new_syms)))
    # demangled name -> (symbol, entry); the parent's after --rename
    old = {renamed(dem[s]): (s, e) for s, e in old_syms.items()}
    new = {dem[s]: (s, e) for s, e in new_syms.items()}
    must = [re.compile(r) for r in a.must_match]
    keys = list(_NOTES)
    lines, bad, same, n_must = [], [], 0, 0
    for name in sorted(set(old) | set(new)):
        (so, o), (sr, r) = old.get(name, (None, None)), new.get(name, (None, None))
        pinned = any(rx.search(name) or any(s and rx.search(s) for s in (so, sr)) for rx in must)
        n_must += pinned
        if o and r and o["body"] == r["body"] and all(o.get(k) == r.get(k) for k in keys):
            same += 1
            continue
        rec = {"kernel": name}
        if so and dem[so] != name:
            rec["parent_name"] = dem[so]
        if not o or not r:
            rec["only_in"] = "result" if r else "parent"
            bad.append(f"{name}: only in the {rec['only_in']}")
        else:
            rec["lines"] = [len(o["body"]), len(r["body"])]
            for k in keys:
                rec[k] = [o.get(k), r.get(k)]
            if pinned:
                bad.append(f"{name}: must be identical")
            if o.get("scratch") == 0 and (r.get("scratch") or 0) > 0:
                bad.append(f"{name}: scratch 0 -> {r.get('scratch')}")
            if (r.get("occupancy") or 0) < (o.get("occupancy") or 0):
                bad.append(f"{name}: occupancy {o.get('occupancy')} -> {r.get('occupancy')}")
        lines.append(rec)
    head = {"note": "device code per kernel, parent against result; pairs are [parent, result]",
            "kernels_parent": len(old), "kernels_result": len(new), "identical": same,
            "differing": len(lines), "must_match": a.must_match, "rename": a.rename,
            "must_match_kernels": n_must,
            "violations": bad}
    print(json.dumps(head))
    for rec in lines:
        print(json.dumps(rec))
    for b in bad:
        print("isa_diff: " + b, file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
