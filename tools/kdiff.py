#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 device code of two build directories:

    tools/kdiff.py [-q] <build dir A> <build dir B> [name-regex]

Every object (*.o) of a directory that holds a .hip_fatbin is unbundled as tools/kres.sh does, and
every kernel of its gfx950 code object gives one record:
  - its name (the mangled symbol);
  - code: the sha256 of its code bytes, exactly st_size bytes from its symbol, so the padding
    between functions and the filler after a unit's last one do not count;
  - kd: the sha256 of its 64-byte kernel descriptor with the code-entry offset (bytes 16-23, which
    depends on where the linker put the code) zeroed;
  - the resource fields tools/kres.sh prints.
Records are keyed and sorted by kernel name, whichever object holds the kernel, so a kernel that
moved to another translation unit is compared with itself.  "= " lines are the same on both sides,
"< " only in (or as in) A, "> " only in (or as in) B.  Objects of the same name on both sides also
get their whole .text / .rodata / .note sha256 compared ("obj" lines): the proof for units that did
not move.  name-regex limits the "= " lines printed (say '_ZN3rtk' for the project's own kernels,
leaving out the several hundred rocPRIM instances); every kernel is still compared and counted, and
a difference is always printed.  -q prints no "= " line and no hash of an equal object: the
differences, then for each object of B how many kernels it holds and how many of them equal A's
kernel of that name (the record to keep of a run; the listing is reproducible).  Exit status 1 when
any kernel, the set of kernels, or a same-named object differs.
A kernel's code can be compared on its own because these code objects have no relocations and no
calls (checked: a code object with a relocation section is an error)."""
import glob
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def code_object(obj, tmp):
    """The gfx950 code object inside obj (bytes and its path), or None without a .hip_fatbin."""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "k.co")
    for p in (fat, co):
        if os.path.exists(p):
            os.remove(p)
    # (an output path of its own: with none, llvm-objcopy rewrites obj in place)
    r = subprocess.run([LLVM + "/llvm-objcopy", "--dump-section=.hip_fatbin=" + fat, obj,
                        os.path.join(tmp, "copy.o")], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return None
    subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=" + TARGET, "--output=" + co], check=True, capture_output=True)
    return open(co, "rb").read(), co


def elf_sections(b):
    """{name: (type, addr, offset, size, link, entsize, index)} of a little-endian ELF64."""
    assert b[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64"
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    raw = []
    for i in range(shnum):
        name, typ, _flags, addr, off, size, link, _info, _align, entsize = struct.unpack_from(
            "<IIQQQQIIQQ", b, shoff + i * shentsize)
        raw.append((name, typ, addr, off, size, link, entsize))
    stro = raw[shstrndx][3]
    secs = {}
    for i, (name, typ, addr, off, size, link, entsize) in enumerate(raw):
        end = b.index(b"\0", stro + name)
        secs[b[stro + name:end].decode()] = (typ, addr, off, size, link, entsize, i)
    return secs


def elf_symbols(b, secs):
    """[(name, value, size, type, shndx)] of .symtab."""
    _typ, _addr, off, size, link, entsize, _i = secs[".symtab"]
    stro = [s for s in secs.values() if s[6] == link][0][2]
    out = []
    for k in range(size // entsize):
        name, info, _other, shndx, value, sz = struct.unpack_from("<IBBHQQ", b, off + k * entsize)
        end = b.index(b"\0", stro + name)
        out.append((b[stro + name:end].decode(), value, sz, info & 15, shndx))
    return out


def resources(co):
    """{kernel name: 'vgpr .. private ..'} from the code object's metadata note, as tools/kres.sh."""
    txt = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for m in re.finditer(r"^ +\.(name|" + "|".join(FIELDS) + r"):\s+(\S+)", txt, re.M):
        k, v = m.group(1), m.group(2)
        if k == "name":
            name = v
        else:
            cur[k] = v
        # (.name sorts before the counts after it and after the segment sizes before it, as in
        # kres.sh: the record is complete at .vgpr_spill_count)
        if k == "vgpr_spill_count":
            out[name] = "vgpr %s spill %s sgpr %s spill %s lds %s private %s" % (
                cur.get("vgpr_count"), cur.get("vgpr_spill_count"), cur.get("sgpr_count"),
                cur.get("sgpr_spill_count"), cur.get("group_segment_fixed_size"),
                cur.get("private_segment_fixed_size"))
            cur = {}
    return out


def scan(build_dir):
    """({kernel: record}, {object: section hashes}, {kernel: its object}) of a build directory."""
    kernels, objects, owner = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
            got = code_object(obj, tmp)
            if got is None:
                continue
            b, co = got
            oname = os.path.basename(obj)
            secs = elf_sections(b)
            for s, v in secs.items():
                if v[0] in (4, 9) and v[3]:  # SHT_RELA / SHT_REL
                    sys.exit("%s: relocation section %s: kernels cannot be compared one by one" % (obj, s))
            objects[oname] = " ".join("%s %s" % (s, sha(b[secs[s][2]:secs[s][2] + secs[s][3]]) if s in secs else "-")
                                      for s in (".text", ".rodata", ".note"))
            syms = elf_symbols(b, secs)
            by_index = {v[6]: v for v in secs.values()}
            where = {n: (val, sz, ndx) for n, val, sz, _t, ndx in syms}
            res = resources(co)
            for n, val, sz, typ, ndx in syms:
                if typ != 2 or n + ".kd" not in where:  # STT_FUNC with a kernel descriptor
                    continue
                _t, addr, off, _s, _l, _e, _i = by_index[ndx]
                code = b[off + val - addr:off + val - addr + sz]
                kval, ksz, kndx = where[n + ".kd"]
                assert ksz == 64, (n, ksz)
                _t, kaddr, koff, _s, _l, _e, _i = by_index[kndx]
                kd = bytearray(b[koff + kval - kaddr:koff + kval - kaddr + 64])
                kd[16:24] = bytes(8)
                rec = "code %s kd %s %s" % (sha(code), sha(bytes(kd)), res.get(n, "no metadata"))
                key = n if n not in kernels else n + "@" + oname  # (a name two objects both define)
                kernels[key] = rec
                owner[key] = oname
    return kernels, objects, owner


def main():
    args = sys.argv[1:]
    quiet = args[:1] == ["-q"]
    args = args[quiet:]
    if len(args) not in (2, 3):
        sys.exit(__doc__)
    (ka, oa, _wa), (kb, ob, wb) = scan(args[0]), scan(args[1])
    listed = re.compile(args[2] if len(args) == 3 else "")
    differ = 0
    for n in sorted(set(ka) | set(kb)):
        if ka.get(n) == kb.get(n):
            if not quiet and listed.search(n):
                print("= %s %s" % (n, ka[n]))
            continue
        differ += 1
        if n in ka:
            print("< %s %s" % (n, ka[n]))
        if n in kb:
            print("> %s %s" % (n, kb[n]))
    for o in sorted(set(oa) & set(ob)):
        same = oa[o] == ob[o]
        differ += not same
        if same and quiet:
            print("obj = %s .text .rodata .note" % o)
        else:
            print("obj %s %s %s" % ("=" if same else "!", o, oa[o] if same else oa[o] + " | " + ob[o]))
    if quiet:
        for o in sorted(ob):
            mine = [n for n in kb if wb[n] == o]
            print("%s: %d kernels, %d equal to A's" % (o, len(mine), sum(ka.get(n) == kb[n] for n in mine)))
    print("objects only in A: %s; only in B: %s" % (" ".join(sorted(set(oa) - set(ob))) or "-",
                                                    " ".join(sorted(set(ob) - set(oa))) or "-"))
    print("%d kernels in A, %d in B, %d differences" % (len(ka), len(kb), differ))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
