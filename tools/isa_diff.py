#!/usr/bin/env python3
"""Are the kernels of two builds the same instruction streams?  For every object of either directory the gfx950 code object is
unbundled and disassembled (llvm-objdump -d); per kernel symbol the instruction text (addresses and encodings stripped) is compared.
  python tools/isa_diff.py [--pooled] OBJDIR_A OBJDIR_B [name-filter ...]
Used to show that a change that adds kernel families leaves the existing instantiations as they were (a parent-commit build against
the branch's), or that a refactor of the launch layer leaves the device code as it was.  Symmetric: exit status 1 when a common kernel
differs, or when an object or a kernel of one build is missing in the other.
--pooled: the kernels are compared over the union of all objects of each build, so one that moved to another object is still found.
They are matched by demangled name with `(anonymous namespace)::` and `fbus::` removed: a kernel's mangled name changes when one of its
argument types changes namespace.  The name filters then select kernels, not objects.
In both modes the alignment padding behind a kernel's last instruction is not part of it."""
import glob, hashlib, os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"


# what fills the gap up to the next kernel's alignment: s_nop, zero bytes (four of them disassemble to this v_cndmask), and "...", which
# llvm-objdump prints for a longer run of zeros
PADDING = ("s_nop 0", "v_cndmask_b32_e32 v0, s0, v0, vcc", "...")


def _digest(body):
    """(sha1, instructions) of a kernel's instruction text without the padding behind its last instruction (a kernel ends in s_endpgm or
    a branch): how much of it there is depends on which kernel the object places next, not on the kernel"""
    while body and body[-1] in PADDING:
        body.pop()
    return hashlib.sha1("\n".join(body).encode()).hexdigest(), len(body)


def _pooled_name(name):
    """a demangled kernel name without the namespaces the kernels and their argument types may move between, and without its parameter
    list (a kernel with C linkage has none)"""
    name = name.replace("(anonymous namespace)::", "").replace("fbus::", "")
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                return name[:i]
    return name


def kernels_of(obj, demangle=False):
    """{symbol: (sha1 of its instruction text, its instructions)}"""
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", f"--input={obj}"], capture_output=True, text=True)
        tgts = [t for t in r.stdout.split() if "gfx950" in t]
        if not tgts:                      # a host object with the fat binary in a section: dump .hip_fatbin first
            fb = os.path.join(td, "fb")
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", f"--input={fb}"], capture_output=True, text=True)
            tgts = [t for t in r.stdout.split() if "gfx950" in t]
            obj = fb
        out = {}
        for i, t in enumerate(tgts):
            co = os.path.join(td, f"co{i}")
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={obj}", f"--targets={t}",
                            f"--output={co}"], check=True)
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn"] + ["--demangle"] * demangle + [co], capture_output=True, text=True).stdout
            name, body = None, []
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    if name is not None:
                        out[name] = _digest(body)
                    name, body = m.group(1), []
                elif name is not None and line.strip():
                    # "\ts_load_dwordx2 s[0:1], ... // 000000001234: ..." -> the instruction alone
                    body.append(re.sub(r"\s*//.*$", "", line).strip())
            if name is not None:
                out[name] = _digest(body)
        return out


def pool_of(objdir):
    """{normalised demangled name: {sha1, ...}} over every object of a build, and the kernel and instruction counts"""
    pool, nk, ni = {}, 0, 0
    for p in sorted(glob.glob(os.path.join(objdir, "*.o"))):
        for k, (h, n) in kernels_of(p, demangle=True).items():
            pool.setdefault(_pooled_name(k), set()).add(h)
            nk += 1; ni += n
    return pool, nk, ni


def main_pooled(a, b, filt):
    (pa, nk, ni), (pb, nkb, nib) = pool_of(a), pool_of(b)
    bad = 0
    for k in sorted(set(pa) | set(pb)):
        if filt and not any(f in k for f in filt):
            continue
        if k not in pa or k not in pb:
            print("only in B:" if k not in pa else "only in A:", k); bad += 1
        elif pa[k] != pb[k]:
            print("differs:", k); bad += 1
    print(f"total: A {nk} kernels, {ni} instructions; B {nkb} kernels, {nib} instructions; {bad} differ")
    sys.exit(1 if bad else 0)


def main():
    if sys.argv[1] == "--pooled":
        main_pooled(sys.argv[2], sys.argv[3], sys.argv[4:])
    a, b, filt = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    nk = ni = 0
    nkb = nib = 0
    names = {os.path.basename(p) for d in (a, b) for p in glob.glob(os.path.join(d, "*.o"))}
    for base in sorted(names):
        if filt and not any(f in base for f in filt):
            continue
        pa, pb = os.path.join(a, base), os.path.join(b, base)
        if not os.path.exists(pa) or not os.path.exists(pb):
            print(f"{base}: missing in {b if os.path.exists(pa) else a}"); bad += 1
            continue
        ka, kb = kernels_of(pa), kernels_of(pb)
        diff = [k for k in ka if k not in kb or ka[k][0] != kb[k][0]]
        extra = [k for k in kb if k not in ka]
        nk += len(ka); ni += sum(v[1] for v in ka.values())
        nkb += len(kb); nib += sum(v[1] for v in kb.values())
        print(f"{base}: {len(ka)} kernels, {sum(v[1] for v in ka.values())} instructions, {len(diff)} differ" +
              (f", {len(extra)} only in B" if extra else ""))
        for k in diff:
            print("   differs:" if k in kb else "   only in A:", k)
        for k in extra:
            print("   only in B:", k)
        bad += len(diff) + len(extra)
    print(f"total: A {nk} kernels, {ni} instructions; B {nkb} kernels, {nib} instructions; {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
