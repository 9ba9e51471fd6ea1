"""tools/kernel_digest.py OBJDIR -> one line per device function of every gfx950 code object under OBJDIR:
   sha1(code bytes) sha1(kernel descriptor or '-') size demangled-name
Sorted, so two builds can be diffed: a source reorganisation that leaves the kernels alone gives the same SET of lines
(python tools/kernel_digest.py p2p_bridge_amd/csrc/build | sort -u, for both trees), and `sort | uniq -d` lists what is
emitted more than once.

Two fields move when a kernel moves to another object although nothing in it changed, and are taken out of the hashes:
  * bytes 16-23 of the kernel descriptor: the descriptor-to-code offset;
  * the literal of  s_getpc_b64 s[n:n+1] / s_add_u32 sn, sn, LIT / s_addc_u32 sn+1, sn+1, LIT : the distance from the
    instruction to a read-only table of the kernel in .rodata (a `constexpr` array indexed at run time, e.g. POS of
    active_lists_kernel). The literal is replaced by what it points at: the table's bytes and the offset into it. A literal
    that does not land in an OBJECT symbol of the code object is left as it is."""
import glob, hashlib, os, struct, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(o, tmp):
    fat, co = os.path.join(tmp, "x.fat"), os.path.join(tmp, "x.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", o], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


def sections(co):
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-W", co], capture_output=True, text=True, check=True).stdout
    secs = {}
    for line in out.splitlines():
        line = line.replace("[ ", "[")
        f = line.split()
        if len(f) > 6 and f[0].startswith("[") and f[0].endswith("]") and f[0][1:-1].isdigit():
            secs[int(f[0][1:-1])] = (f[1], int(f[3], 16), int(f[4], 16))  # name, addr, file offset
    return secs


def position_independent(blob, addr, tables):
    """blob with every pc-relative table reference replaced by zeros, + (table bytes, offset) of each reference"""
    words = list(struct.unpack("<%dI" % (len(blob) // 4), blob[:len(blob) // 4 * 4]))
    refs = []
    for i in range(len(words) - 4):
        w = words[i]
        if w & 0xff80ffff != 0xbe801c00:  # s_getpc_b64 s[n:n+1]
            continue
        n = (w >> 16) & 0x7f
        if words[i + 1] != (0x8000ff00 | n << 16 | n) or words[i + 3] != (0x8200ff00 | (n + 1) << 16 | (n + 1)):
            continue
        lit = struct.unpack("<q", struct.pack("<II", words[i + 2], words[i + 4]))[0]
        target = addr + 4 * (i + 1) + lit  # s_getpc_b64 returns the address of the instruction behind it
        for start, data in tables:
            if start <= target < start + len(data):
                refs.append(data + struct.pack("<q", target - start))
                words[i + 2] = words[i + 4] = 0
                break
    return struct.pack("<%dI" % len(words), *words) + blob[len(words) * 4:] + b"".join(refs)


def main(objdir):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(glob.glob(os.path.join(objdir, "*.o"))):
            co = code_object(o, tmp)
            data = open(co, "rb").read()
            secs = sections(co)
            sym = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
            funcs, kds, tables = {}, {}, []
            for line in sym.splitlines():
                f = line.split()
                if len(f) < 8 or not f[0].endswith(":") or not f[6].isdigit():
                    continue
                val, size, typ, ndx, name = int(f[1], 16), int(f[2]), f[3], int(f[6]), f[7]
                secname, addr, off = secs[ndx]
                blob = data[off + val - addr: off + val - addr + size]
                if typ == "FUNC":
                    funcs[name] = (blob, val)
                elif typ == "OBJECT" and name.endswith(".kd"):
                    kds[name[:-3]] = blob
                elif typ == "OBJECT" and secname == ".rodata":
                    tables.append((val, blob))
            for name, (blob, val) in funcs.items():
                kd = kds.get(name)
                rows.append((name, hashlib.sha1(position_independent(blob, val, tables)).hexdigest()[:16],
                             hashlib.sha1(kd[:16] + kd[24:]).hexdigest()[:16] if kd else "-", len(blob)))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.splitlines()
    for (n, h, k, s), d in sorted(zip(rows, names), key=lambda x: (x[1], x[0][1])):
        print(h, k, s, d)


if __name__ == "__main__":
    main(sys.argv[1])
