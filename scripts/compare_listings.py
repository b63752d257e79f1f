"""Compare the device functions of two hipcc -save-temps listings (mpc_api-hip-amdgcn-amd-amdhsa-gfx950.s) body for body.

Usage: python scripts/compare_listings.py OLD.s NEW.s
Every kernel present in both listings must have the same instructions once label numbers, comments and directives that only name
sections or sizes are ignored.  Kernels only in NEW (new instantiations) are listed; kernels only in OLD are an error.  Exit 1 on any difference.
A kernel that gained a trailing `bool` template parameter whose default (false) keeps the old code -- the REF parameter of the per-stage reference,
the IPAR parameter of the per-instance parameters, the OSEL parameter of the obstacle masks -- is matched to its old name: rti_*_kernel<..., false> and linearize_kernel<..., false>.
"""
import re
import sys

_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)*")


def bodies(path):
    out, name, cur = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            if name is not None:
                out[name] = cur
            name, cur = m.group(1), []
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith((".size", ".section", ".p2align", ".type", ".globl", ".protected", ".Lfunc_end", ".set", ".amdgpu", ".text",
                                  ".amdhsa_", ".end_amdhsa", ".rodata")):
            if s.startswith(".Lfunc_end"):
                out[name] = cur; name, cur = None, []
            continue
        cur.append(_LABEL.sub(".L", s))
    if name is not None:
        out[name] = cur
    return {k: v for k, v in out.items() if k.startswith("_Z") and v and any(not x.startswith(".") for x in v)}


_OFF = re.compile(r"^(s_load\w*|s_buffer_load\w*) (.*), (0x[0-9a-f]+)$")


def arg_shift(x, y):
    """the kernel-argument offset by which two scalar loads differ, or None (argument structs grew: loads of arguments behind it move)"""
    a, b = _OFF.match(x), _OFF.match(y)
    if not a or not b or a.group(1) != b.group(1) or a.group(2) != b.group(2):
        return None
    return int(b.group(3), 16) - int(a.group(3), 16)


def new_name(k, b):
    """the NEW symbol of OLD kernel k: itself, or its instantiation with one more template argument `false`"""
    if k in b:
        return k
    if "EEEvNS_7KParamsE" in k:                         # rti_*_kernel<...>(KParams), linearize_kernel<...>(KParams, ...) -> the same with <..., false>
        c = k.replace("EEEvNS_7KParamsE", "ELb0EEEvNS_7KParamsE", 1)
        if c in b:
            return c
    m = re.match(r"^(_ZN3mpc\d+\w+?)E(NS_7KParamsE.*)$", k)   # a non-template kernel that became a template: match on the base name
    if m:
        for c in b:
            if c.startswith(m.group(1) + "ILb0EEEv"):
                return c
    return None


def main(old, new):
    a, b = bodies(old), bodies(new)
    bad, used = 0, set()
    for k0 in sorted(a):
        k = new_name(k0, b)
        used.add(k)
        if k is None:
            print("missing in NEW:", k0); bad += 1
            continue
        k, kb = k0, k
        if a[k] != b[kb] and len(a[k]) == len(b[kb]):
            shifts = {arg_shift(x, y) for x, y in zip(a[k], b[kb]) if x != y}
            if None not in shifts:
                print(f"args:    {k}: identical except kernel-argument offsets moved by {sorted(shifts)} bytes (arguments behind KParams)")
                continue
        if a[k] != b[kb]:
            n = next(i for i, (x, y) in enumerate(zip(a[k] + [""], b[kb] + [""])) if x != y)
            print(f"DIFFERS: {k} ({len(a[k])} vs {len(b[kb])} lines; first at {n}: {a[k][n] if n < len(a[k]) else ''!r} vs {b[kb][n] if n < len(b[kb]) else ''!r})")
            bad += 1
    added = sorted(set(b) - used)
    print(f"{len(a)} functions in OLD, {len(used - {None})} compared, {bad} differ or are missing; {len(added)} only in NEW")
    for k in added:
        print("  new:", k)
    return 1 if bad else 0


def _unused(old, new):
    a, b = bodies(old), bodies(new)
    bad = 0
    for k in sorted(a):
        if k not in b:
            print("missing in NEW:", k); bad += 1
        elif a[k] != b[k]:
            n = next(i for i, (x, y) in enumerate(zip(a[k] + [""], b[k] + [""])) if x != y)
            print(f"DIFFERS: {k} ({len(a[k])} vs {len(b[k])} lines; first at {n}: {a[k][n] if n < len(a[k]) else ''!r} vs {b[k][n] if n < len(b[k]) else ''!r})")
            bad += 1
    added = sorted(set(b) - set(a))
    print(f"{len(a)} functions in OLD, {len(set(a) & set(b))} compared, {bad} differ or are missing; {len(added)} only in NEW")
    for k in added:
        print("  new:", k)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
