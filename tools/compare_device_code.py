#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?  (No GPU needed.)

    python tools/compare_device_code.py OLD_TREE NEW_TREE [--work DIR] [-j N] [--rename OLD_NAME=NEW_NAME ...]

For each tree every .hip of probreg_amd/csrc is compiled with exactly the command its Makefile would run (taken from
`make -n -B`) plus `--cuda-device-only --no-gpu-bundle-output`, which leaves one plain gfx950 ELF per file.  The kernels of an
ELF are its FUNC symbols that have a `.kd` descriptor beside them; each one is disassembled on its own
(`llvm-objdump -d --disassemble-symbols=NAME`), addresses and encodings are stripped, and the instruction lists of the two
trees are compared under the kernel's mangled name - whichever file it lives in (a name that several files define, as kernels in
anonymous namespaces may, is compared as the sorted list of its definitions).  Exit status 0: every kernel of OLD exists
in NEW with identical instructions and NEW has no others.
"""
import argparse
import concurrent.futures as cf
import os
import re
import shlex
import subprocess
import sys

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def compile_commands(csrc):
    out = subprocess.run(["make", "-n", "-B", "-C", csrc], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    cmds = {}
    for line in out.splitlines():
        words = shlex.split(line)
        if "-c" in words and "-o" in words:
            src = words[words.index("-c") + 1]
            cmds[src] = words
    return cmds


def device_elf(csrc, src, words, work):
    elf = os.path.join(work, src.replace(".hip", ".elf"))
    words = list(words)
    words[words.index("-o") + 1] = elf
    subprocess.run(words + ["--cuda-device-only", "--no-gpu-bundle-output"], check=True, cwd=csrc)
    return elf


def kernels_of(elf):
    out = subprocess.run([os.path.join(ROCM_LLVM, "llvm-readelf"), "-sW", elf], check=True, stdout=subprocess.PIPE,
                         universal_newlines=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if len(l.split()) >= 8}
    return sorted(n for n in names if n + ".kd" in names)


def instructions(elf, name):
    out = subprocess.run([os.path.join(ROCM_LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                          "--disassemble-symbols=" + name, elf], check=True, stdout=subprocess.PIPE,
                         universal_newlines=True).stdout
    body = []
    for line in out.splitlines():
        line = re.sub(r"\s*//.*$", "", line).strip()  # "// 0000000012A4: ..." address / encoding comments
        # ("...": zero padding objdump skips behind the last symbol of a section - no instruction)
        # (the kernel's own label goes too: a kernel compared under --rename differs in nothing else)
        if line and line not in ("...", "<%s>:" % name) and not line.startswith(("Disassembly", elf)) and "file format" not in line:
            body.append(line)
    while body and body[-1] == "s_nop 0":  # alignment padding behind the program's end: s_nop before another kernel, zeros at
        body.pop()                         # the end of the section - which of the two depends on the kernel's place in the file
    return body


def tree_kernels(tree, work, jobs):
    csrc = os.path.join(tree, "probreg_amd", "csrc")
    os.makedirs(work, exist_ok=True)
    cmds = compile_commands(csrc)
    with cf.ThreadPoolExecutor(jobs) as pool:
        elfs = list(pool.map(lambda kv: (kv[0], device_elf(csrc, kv[0], kv[1], work)), sorted(cmds.items())))
    found = {}
    for src, elf in elfs:
        for name in kernels_of(elf):
            # (kernels in anonymous namespaces: the same mangled name may exist in several files - keep them all)
            found.setdefault(name, []).append((instructions(elf, name), src))
    return {name: sorted(defs) for name, defs in found.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--work", default="/tmp/compare_device_code")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="a kernel whose mangled name changed on purpose (say, it left an anonymous namespace to be declared "
                         "in a header): OLD of the old tree is compared with NEW of the new one")
    a = ap.parse_args()
    old = tree_kernels(a.old, os.path.join(a.work, "old"), a.j)
    new = tree_kernels(a.new, os.path.join(a.work, "new"), a.j)
    for pair in a.rename:
        was, now = pair.split("=")
        if was in old and was not in new and now in new and now not in old:
            print("renamed  %s -> %s" % (was, now))
            old[now] = old.pop(was)
    bad = 0
    files = lambda defs: ", ".join(src for _, src in defs)
    for name in sorted(set(old) | set(new)):
        if name not in new:
            print("REMOVED  %s (%s)" % (name, files(old[name])))
        elif name not in old:
            print("ADDED    %s (%s)" % (name, files(new[name])))
        elif [ins for ins, _ in old[name]] != [ins for ins, _ in new[name]]:
            print("DIFFERS  %s (%s -> %s)" % (name, files(old[name]), files(new[name])))
        else:
            if sorted(files(old[name])) != sorted(files(new[name])):
                print("moved    %s: %s -> %s" % (name, files(old[name]), files(new[name])))
            continue
        bad += 1
    print("%d kernels in the old tree, %d in the new one, %d added / removed / different" %
          (sum(map(len, old.values())), sum(map(len, new.values())), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
