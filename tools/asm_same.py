#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds of one translation unit, kernel by kernel.

    hipcc <the Makefile's flags for the file> --cuda-device-only -S -x hip FILE -o old.s   (at the parent)
    hipcc ...                                                              -o new.s   (at the change)
    tools/asm_same.py old.s new.s

Every function of old.s is looked up in new.s by its mangled name (a trailing defaulted
`false` template argument, Lb0E, is dropped, so a kernel that gained `bool CAUSAL = false`
still matches, and the dense family's mask argument is reduced to one spelling: key()) and its body (the lines between its label and its .Lfunc_end, with the function's
own mangled name and the compiler's local label numbers normalised) is compared.  Prints one
line per function that differs or is missing and a final count; exit status 1 if any differs.
"""
from __future__ import annotations

import re
import sys


def functions(path: str) -> dict:
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        if name is None:
            m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
            if m:
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].rstrip()       # drop comments
        # (the kernel descriptor sits inside the function's extent and is compared too, except
        # the size of the by-value parameter struct, which grows when a field is appended)
        if s and ".amdhsa_kernarg_size" not in s:
            body.append(s)
    return out


def key(mangled: str) -> str:
    """The mangled name with its dense-family mask argument in one canonical spelling: nothing
    for no mask, @M1 causal, @M2 local.  Reduces to it the old trailing `bool CAUSAL, bool LOCAL`
    pair (defaults are mangled too), the new trailing `DenseMask MASK`, and the old forward
    wrapper names causal_fwd_* / local_fwd_* (now dense_fwd_*<..., MASK>)."""
    k = re.sub(r"LNS_9DenseMaskE([012])E(?=EEv)", lambda m: "@M" + m.group(1), mangled)
    k = re.sub(r"Lb([01])ELb([01])E(?=EEv)",
               lambda m: {"00": "@M0", "10": "@M1", "01": "@M2"}.get(m.group(1) + m.group(2), m.group(0)), k)
    m = re.match(r"(_ZN2fa)(\d+)(causal|local)(_fwd_\w+)$", k)
    if m and int(m.group(2)) < len(m.group(3) + m.group(4)):
        n = int(m.group(2)) - len(m.group(3))              # the name's characters after the mask's word
        rest = m.group(4)
        k = "%s%ddense%s" % (m.group(1), n + 5, rest[:n]) + re.sub(r"(?=EEv)", "@M1" if m.group(3) == "causal" else "@M2", rest[n:], count=1)
    k = k.replace("@M0", "")
    return re.sub(r"(Lb0E)+(?=EEv)", "", k)


def norm(body, own: str):
    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ".L", l.replace(own, "@")) for l in body]


def main(old_s: str, new_s: str) -> int:
    old, new = functions(old_s), functions(new_s)
    by_key = {key(n): n for n in new}
    same = diff = missing = 0
    for n, body in old.items():
        k = key(n)
        if k not in by_key:
            print("MISSING  ", n)
            missing += 1
            continue
        m = by_key[k]
        if norm(body, n) == norm(new[m], m):
            same += 1
        else:
            print("DIFFERS  ", n)
            diff += 1
    print(f"{old_s} -> {new_s}: {len(old)} functions at the parent: {same} identical, {diff} differ, "
          f"{missing} missing; {len(new) - len(by_key.keys() & {key(n) for n in old})} new")
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
