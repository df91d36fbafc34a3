#!/usr/bin/env python3
"""Instruction counts of one kernel in a `hipcc -S` listing, by mnemonic prefix.

    tools/isa_sections.py LISTING.s MANGLED_NAME [--ranges TABLE.json] [--key NAME]

Prints, for the whole kernel and for every labelled range of the table, how
many instructions it holds and how they split by the prefix of the mnemonic:

    scalar   s_*  (other than branches)
    valu     v_*
    vmem     global_* buffer_* flat_* scratch_*
    lds      ds_*
    branch   s_branch* s_cbranch* s_setpc* s_swappc* s_endpgm*
    other    anything else

It counts by prefix and does nothing else: it knows no particular opcode.

A table is a JSON object {key: [[range name, first label, last label], ...]};
`--key` picks the entry (default: the mangled name).  A range runs from the
line of its first label up to, not including, the line of its last label; an
empty first label is the kernel's start, an empty last label its end.  Label
numbers belong to one build of one compiler, so a table is committed beside
the listing's figures it was used for (profiles/*/ranges_*.json).
"""
import argparse
import json
import re
import sys

CLASSES = ("scalar", "valu", "vmem", "lds", "branch", "other")
_BRANCH = ("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm")
_VMEM = ("global_", "buffer_", "flat_", "scratch_")
_LABEL = re.compile(r"^([.\w$]+):")
_MNEMONIC = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def classify(mnemonic):
    """The class of a mnemonic, by its prefix."""
    if mnemonic.startswith(_BRANCH):
        return "branch"
    if mnemonic.startswith("s_"):
        return "scalar"
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith(_VMEM):
        return "vmem"
    if mnemonic.startswith("ds_"):
        return "lds"
    return "other"


def kernel_lines(text, name):
    """The listing's lines from `name:` up to its `.Lfunc_end` label."""
    lines = text.splitlines()
    start = None
    for i, line in enumerate(lines):
        if start is None:
            if line.startswith(name + ":"):
                start = i + 1
        elif line.startswith(".Lfunc_end"):
            return lines[start:i]
    if start is None:
        raise KeyError("no function %s in the listing" % name)
    return lines[start:]


def parse(lines):
    """-> (items, labels): items is the list of instruction classes in order,
    labels maps a label to the index of the first instruction after it."""
    items, labels = [], {}
    for line in lines:
        m = _LABEL.match(line)
        if m:
            labels[m.group(1)] = len(items)
            continue
        code = line.split(";", 1)[0]
        if not code.strip() or code.lstrip().startswith("."):
            continue
        m = _MNEMONIC.match(code)
        if m:
            items.append(classify(m.group(1)))
    return items, labels


def count(items):
    out = dict.fromkeys(CLASSES, 0)
    for c in items:
        out[c] += 1
    out["total"] = len(items)
    return out


def sections(text, name, ranges=()):
    """[(range name, counts)], the whole kernel first."""
    items, labels = parse(kernel_lines(text, name))
    out = [("kernel", count(items))]
    for rname, first, last in ranges:
        for lab in (first, last):
            if lab and lab not in labels:
                raise KeyError("range %s: no label %s in %s" % (rname, lab, name))
        a = labels[first] if first else 0
        b = labels[last] if last else len(items)
        if b < a:
            raise ValueError("range %s: %s comes after %s" % (rname, first, last))
        out.append((rname, count(items[a:b])))
    return out


def render(rows):
    head = "%-28s %7s" % ("range", "total") + "".join(" %7s" % c for c in CLASSES)
    body = ["%-28s %7d" % (n, c["total"]) + "".join(" %7d" % c[k] for k in CLASSES) for n, c in rows]
    return "\n".join([head] + body)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--ranges")
    ap.add_argument("--key")
    a = ap.parse_args(argv)
    ranges = ()
    if a.ranges:
        with open(a.ranges) as f:
            ranges = json.load(f).get(a.key or a.kernel, ())
    with open(a.listing) as f:
        print(render(sections(f.read(), a.kernel, ranges)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
