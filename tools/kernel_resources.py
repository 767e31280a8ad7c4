"""Registers / scratch / instruction counts of every step-kernel variant in the built library: carves the gfx950 code objects out of libsmj.so's
fat binary (clang offload bundle: ELF images after the bundle header) and reads their metadata notes.  No GPU needed.
Usage: python tools/kernel_resources.py [--digest] [path/to/libsmj.so]
--digest: one line per kernel symbol of EVERY code object (not only the step kernels) with the SHA-256 of the kernel's machine code
bytes, the SHA-256 of its 64-byte kernel descriptor (<name>.kd) and the metadata that sizes a launch, and one line per code object with
the SHA-256 of its whole .text section.  Two libraries whose sorted listings are equal line for line run the same device code
(profiles/build_table_isa_digest.txt)."""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGEST_META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
               "group_segment_fixed_size", "kernarg_segment_size")


def code_objects(blob):
    """The AMDGPU ELF images inside the library, in file order."""
    pos = 0
    while True:
        pos = blob.find(b"\x7fELF\x02\x01\x01\x40", pos)   # ELF64, little endian, OS ABI 64 = AMDGPU HSA
        if pos < 0:
            return
        # section header table offset + count * size bounds the image
        shoff = int.from_bytes(blob[pos + 0x28:pos + 0x30], "little")
        shentsize = int.from_bytes(blob[pos + 0x3A:pos + 0x3C], "little")
        shnum = int.from_bytes(blob[pos + 0x3C:pos + 0x3E], "little")
        end = pos + shoff + shentsize * shnum
        yield blob[pos:end]
        pos = end


def kernel_notes(image, d, n):
    """{kernel name: metadata block (text)} of one code object, from its notes."""
    path = os.path.join(d, f"co{n}.o")
    open(path, "wb").write(image)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", path], capture_output=True, text=True).stdout
    blocks = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", out)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            blocks[name.group(1)] = ".agpr_count: " + blk
    return blocks


def instruction_counts(d, n):
    """{symbol: (instructions, v_writelane, v_readlane, branches)} of the code object kernel_notes wrote as co<n>.o, from its disassembly:
    the size of a kernel in instructions, how many of them spill / reload a scalar register through a VGPR lane, and its branches."""
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", os.path.join(d, f"co{n}.o")], capture_output=True, text=True).stdout
    counts, cur = {}, None
    for line in out.split("\n"):
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = counts.setdefault(m.group(1), [0, 0, 0, 0])
        elif cur is not None and "//" in line:
            op = line.split()[0]
            cur[0] += 1
            cur[1] += op.startswith("v_writelane")
            cur[2] += op.startswith("v_readlane")
            cur[3] += op.startswith(("s_cbranch", "s_branch"))
    return counts


def symbol_bytes(image):
    """{symbol name: its bytes in the image} for every defined symbol with a size (functions, kernel descriptors)."""
    shoff, = struct.unpack_from("<Q", image, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", image, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", image, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, offset, size, link, info, align, entsize
    out = {}
    for s in sec:
        if s[1] != 2:   # SHT_SYMTAB
            continue
        strtab = sec[s[6]]
        for off in range(s[4], s[4] + s[5], 24):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", image, off)
            if st_size == 0 or st_shndx == 0 or st_shndx >= shnum or sec[st_shndx][1] == 8:   # undefined / special / SHT_NOBITS
                continue
            e = image.index(b"\0", strtab[4] + st_name)
            name = image[strtab[4] + st_name:e].decode()
            start = sec[st_shndx][4] + st_value - sec[st_shndx][3]
            out[name] = image[start:start + st_size]
    for s in sec:   # and the whole .text of the code object: device functions a kernel calls without inlining them are in here too
        e = image.index(b"\0", sec[shstrndx][4] + s[0])
        if image[sec[shstrndx][4] + s[0]:e] == b".text":
            out[".text"] = image[s[4]:s[4] + s[5]]
    return out


def main(so, digest=False):
    blob = open(so, "rb").read()
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for n, image in enumerate(code_objects(blob)):
            syms = symbol_bytes(image) if digest else {}
            notes = kernel_notes(image, d, n)
            icount = instruction_counts(d, n) if not digest and any("step_kernel" in k for k in notes) else {}
            if digest and notes:
                rows.append(f"{min(notes)} (.text of its code object) {len(syms['.text'])} B sha256 {hashlib.sha256(syms['.text']).hexdigest()}")
            for name, blk in notes.items():
                g = lambda k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [0, "?"])[1]
                if digest:
                    code, kd = syms[name], syms[name + ".kd"]
                    rows.append(f"{name} code {len(code)} B sha256 {hashlib.sha256(code).hexdigest()} kd sha256 {hashlib.sha256(kd).hexdigest()} "
                                + " ".join(f"{k} {g(k)}" for k in DIGEST_META))
                elif "step_kernel" in name:
                    rows.append(f"{name[:48]:48s} agpr {g('agpr_count'):>4s} vgpr {g('vgpr_count'):>4s} sgpr_spill {g('sgpr_spill_count'):>4s} "
                                f"vgpr_spill {g('vgpr_spill_count'):>4s} scratch_bytes_per_lane {g('private_segment_fixed_size'):>5s} "
                                + "instructions {:6d} v_writelane {:5d} v_readlane {:5d} branches {:5d}".format(*icount.get(name, [0, 0, 0, 0])))
    for r in sorted(rows if digest else set(rows)):
        print(r)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--digest"]
    main(args[0] if args else os.path.join(ROOT, "stretch_mujoco_amd", "libsmj.so"), digest="--digest" in sys.argv[1:])
