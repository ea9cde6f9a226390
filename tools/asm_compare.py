#!/usr/bin/env python3
"""Are the kernels of two builds the same code?  Reads two build/asm trees (make -C gym_soccer_littman94_amd/csrc asm:
one .s per translation unit, resource_usage.txt with all units' remarks) and nothing else.
Usage: tools/asm_compare.py BEFORE_DIR AFTER_DIR
Checks, and exits non-zero unless all hold:
  * no kernel is emitted by two units of one tree (each unit is its own code object);
  * both trees hold the same set of kernels;
  * per kernel the compiler's resource remarks (registers, spills, scratch, LDS, occupancy) are equal;
  * per kernel the instruction sequence is equal, comments and the numbers of local labels aside."""
import glob, os, re, sys

def kernels(tree):
    """{kernel: (unit, [instruction, ...])} from the .amdhsa_kernel symbols of every .s file; duplicates are reported"""
    out, dup = {}, []
    for path in sorted(glob.glob(os.path.join(tree, "*.s"))):
        text = open(path).read()
        names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
        name, body, labels = None, [], {}
        for line in text.split("\n"):
            m = re.match(r"^(\w+):", line)
            if name is None:
                if m and m.group(1) in names: name, body, labels = m.group(1), [], {}      # labels: numbered as they appear
                continue
            if line.startswith(".Lfunc_end"):
                if name in out: dup.append((name, out[name][0], os.path.basename(path)))
                out[name] = (os.path.basename(path), body); name = None
                continue
            ins = re.sub(r"\s+", " ", line.split(";")[0]).strip()
            if ins and (not ins.startswith(".") or re.match(r"^\.LBB\d+_\d+:", ins)):
                body.append(re.sub(r"\.LBB\d+_\d+", lambda m: "L%d" % labels.setdefault(m.group(0), len(labels)), ins))
    return out, dup

def resources(tree):
    """{kernel: {remark: value}} from resource_usage.txt"""
    out, cur = {}, None
    for line in open(os.path.join(tree, "resource_usage.txt")):
        m = re.search(r"remark: (.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m: continue
        key, _, val = m.group(1).strip().partition(":")
        if key == "Function Name": cur = out.setdefault(val.strip(), {})
        elif cur is not None: cur[key.strip()] = val.strip()
    return out

def main(before, after):
    bad = 0
    (ka, da), (kb, db) = kernels(before), kernels(after)
    ra, rb = resources(before), resources(after)
    for tree, dup in ((before, da), (after, db)):
        for name, u1, u2 in dup: print("TWICE in %s: %s (%s and %s)" % (tree, name, u1, u2)); bad += 1
    for tree, k, r in ((before, ka, ra), (after, kb, rb)):
        if set(k) != set(r): print("%s: the .s files and the remarks name different kernels: %s" % (tree, sorted(set(k) ^ set(r))[:5])); bad += 1
    for name in sorted(set(ka) - set(kb)): print("ONLY BEFORE: %s" % name); bad += 1
    for name in sorted(set(kb) - set(ka)): print("ONLY AFTER:  %s" % name); bad += 1
    for name in sorted(set(ka) & set(kb)):
        if ra.get(name) != rb.get(name):
            print("RESOURCES differ: %s\n  before %s\n  after  %s" % (name, ra.get(name), rb.get(name))); bad += 1
        a, b = ka[name][1], kb[name][1]
        if a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("CODE differs: %s (%d / %d instructions), first at %d:\n  before %s\n  after  %s"
                  % (name, len(a), len(b), i, a[i:i + 3], b[i:i + 3])); bad += 1
    units = sorted(set(u for u, _ in kb.values()))
    print("%d kernels before, %d after (%s); %d findings" % (len(ka), len(kb), ", ".join(
          "%s %d" % (u, sum(1 for v in kb.values() if v[0] == u)) for u in units), bad))
    return 1 if bad else 0

if __name__ == "__main__":
    if len(sys.argv) != 3: sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
