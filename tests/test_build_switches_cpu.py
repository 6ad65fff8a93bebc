"""The compile-time switches the kernel sources take (-D overrides, zonos_amd.build.build_variant) are
exactly the ones DESIGN.md's "Build switches" table lists, and there are at most 16 of them: an
experiment that is not kept leaves the sources with its switch."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SWITCHES = 16


def _source_switches():
    """Names a -D can override: `#ifndef ZK_X` followed by `#define ZK_X`, or tested by `#ifdef ZK_X` /
    `defined(ZK_X)`. (A plain `#if ZK_X` only reads a name one of those makes overridable.)"""
    files = sorted(glob.glob(os.path.join(ROOT, "zonos_amd", "csrc", "*")))
    files.append(os.path.join(ROOT, "include", "zonos_hip.h"))
    names = set()
    for path in files:
        with open(path, encoding="utf-8") as f:
            lines = f.read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*ifndef\s+(ZK_[A-Z0-9_]+)", line)
            if m:
                body = []
                for nxt in lines[i + 1:]:
                    if re.match(r"\s*#\s*(endif|else|elif)", nxt):
                        break
                    body.append(nxt)
                if any(re.match(r"\s*#\s*define\s+%s\b" % m.group(1), b) for b in body):
                    names.add(m.group(1))
            m = re.match(r"\s*#\s*ifdef\s+(ZK_[A-Z0-9_]+)", line)
            if m:
                names.add(m.group(1))
            if re.match(r"\s*#\s*(if|elif)\b", line):
                names.update(re.findall(r"defined\s*\(?\s*(ZK_[A-Z0-9_]+)", line))
    return names


def _design_switches():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    m = re.search(r"^#+ Build switches\s*$(.*?)(?=^#+ )", text, re.M | re.S)
    assert m, "DESIGN.md has no 'Build switches' section"
    return set(re.findall(r"^\|\s*`(ZK_[A-Z0-9_]+)`", m.group(1), re.M))


def test_build_switches_match_design_table():
    src, doc = _source_switches(), _design_switches()
    assert src == doc, f"only in the sources: {sorted(src - doc)}; only in DESIGN.md: {sorted(doc - src)}"
    assert len(src) <= MAX_SWITCHES, f"{len(src)} overridable switches (at most {MAX_SWITCHES}): {sorted(src)}"
