#!/usr/bin/env python3
"""Are the kernels of two builds the same instruction streams?  For every object of either directory the gfx950 code object is
unbundled and disassembled (llvm-objdump -d); per kernel symbol the instruction text (addresses and encodings stripped) is compared.
  python tools/isa_diff.py OBJDIR_A OBJDIR_B [name-filter ...]
Used to show that a change that adds kernel families leaves the existing instantiations as they were (a parent-commit build against
the branch's), or that a refactor of the launch layer leaves the device code as it was.  Symmetric: exit status 1 when a common kernel
differs, or when an object or a kernel of one build is missing in the other."""
import glob, hashlib, os, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels_of(obj):
    """{symbol: sha1 of its instruction text}"""
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
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            name, body = None, []
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    if name is not None:
                        out[name] = (hashlib.sha1("\n".join(body).encode()).hexdigest(), len(body))
                    name, body = m.group(1), []
                elif name is not None and line.strip():
                    # "\ts_load_dwordx2 s[0:1], ... // 000000001234: ..." -> the instruction alone
                    body.append(re.sub(r"\s*//.*$", "", line).strip())
            if name is not None:
                out[name] = (hashlib.sha1("\n".join(body).encode()).hexdigest(), len(body))
        return out


def main():
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
