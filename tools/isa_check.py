#!/usr/bin/env python3
"""Build-time ISA check of the pipelined bf16 GEMM kernels (tests/test_isa.py runs it on the objects of the built library).

The K loops of gemm_bf16_nt_pipe_kernel / gemm_bf16_tn_kernel issue their LDS-DMA from inline asm the compiler's s_waitcnt pass cannot see,
and rely on two things no compiler pass guarantees:
  1. NO compiler-inserted `s_waitcnt vmcnt` inside the K loop: at run time such a wait also drains the DMA pieces in flight (hardware vmcnt
     counts them) -- the loop then runs at the speed of un-prefetched loads.  Scratch reloads, epilogue loads left "pending" across the tile
     loop's back edge and LDS-DMA builtins all produce them.  Exactly ONE vmcnt wait per K-tile iteration is the schedule's own (hand-over).
  2. M0 is written ONLY by the asm DMA statements (`s_mov_b32 m0, sN` directly followed by `s_nop` + `buffer_load ... lds`): continuation
     pieces reuse the M0 value of the group's first piece across MFMAs, barriers and epilogue code.

The streamed attention kernels (csrc/attn_stream.hip) issue the same asm DMA in their chunk loops; their check (check_stream) reads the WHOLE loop.

    python tools/isa_check.py <object.o> [...]        # prints one line per kernel, exit code 1 on a violation
"""
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def disassemble(obj: str) -> str:
    with tempfile.TemporaryDirectory() as td:
        co, fb = f"{td}/dev.co", f"{td}/fat.bin"
        # the fat binary of a HIP object; the explicit output file keeps llvm-objcopy from rewriting `obj` in place (which would bump its
        # mtime and make build.py skip the next recompile of an edited source)
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, f"{td}/copy.o"], capture_output=True, text=True, check=True)
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}", "--unbundle"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout


def kernels(asm: str):
    cur, body = None, []
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            if cur:
                yield cur, body
            cur, body = m.group(1), []
        elif cur and line.strip():
            body.append(line.strip())
    if cur:
        yield cur, body


def check(name: str, body):
    ins = [re.sub(r"\s*//.*", "", l) for l in body]
    mf = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
    if not mf:
        return None
    lo, hi = mf[0], mf[-1]
    # the K loop = first to last MFMA (the epilogue holds none)
    waits = [l for l in ins[lo:hi + 1] if l.startswith("s_waitcnt") and "vmcnt" in l]
    scratch = [l for l in ins[lo:hi + 1] if l.startswith("scratch_")]
    bad_m0 = []
    for i, l in enumerate(ins):
        ops = l.split(None, 1)
        dst = ops[1].split(",")[0].strip() if len(ops) > 1 else ""
        if dst == "m0" or l.startswith(("s_movrel", "s_set_gpr_idx")):
            nxt = ins[i + 1:i + 3]
            ok = l.startswith("s_mov_b32 m0, s") and len(nxt) == 2 and nxt[0].startswith("s_nop") and nxt[1].startswith("buffer_load_dwordx4") and nxt[1].rstrip().endswith("lds")
            if not ok:
                bad_m0.append(l)
    ok = len(waits) == 1 and not scratch and not bad_m0
    return ok, f"{'ok  ' if ok else 'FAIL'} vmcnt waits in K loop {len(waits)} (want 1), scratch ops in K loop {len(scratch)}, foreign M0 writes {len(bad_m0)}  {name[:110]}"


def check_stream(name: str, body):
    """The streamed attention kernels (csrc/attn_stream.hip): the same two guarantees, counted over the WHOLE chunk loop -- from the target of its
    back edge to the branch, not only between the first and the last MFMA: a compiler wait in front of the first product of an iteration (a
    global load consumed at the loop head) drains the chunk just put in flight as surely as one between two products.  The compiler rotates these
    loops, so an iteration is read in the order it runs: from the first LDS-DMA issue of the loop round to the instruction in front of it.  Wanted:
    every `s_waitcnt vmcnt` of the iteration (the ring's own, and a compiler's for a small load it hands to LDS there) BEHIND the last LDS read
    of the iteration -- the chunk's operands are all in registers by then; the scheduler may leave a few register-only MFMAs behind the wait --
    and at least the ring's one; no scratch access; no foreign M0 write."""
    rows = []
    for l in body:
        m = re.match(r"(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)", l)
        if not m:
            continue
        ins, rest = m.group(1).strip(), m.group(3)
        t = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>", rest) if ins.startswith(("s_cbranch", "s_branch")) else None
        rows.append((int(m.group(2), 16), ins, int(t.group(1), 16) if t else None))
    if not any(ins.startswith("v_mfma") for _, ins, _ in rows):
        return None
    base, loop = rows[0][0], None
    for i, (addr, ins, t) in enumerate(rows):
        if t is None or base + t > addr:
            continue   # not a back edge
        lo = next(j for j, r in enumerate(rows) if r[0] >= base + t)
        span = rows[lo:i + 1]
        if any(r[1].startswith("v_mfma") for r in span) and (loop is None or len(span) > len(loop)):
            loop = span    # the outermost loop that holds the products
    if loop is None:
        return False, f"FAIL no loop around the MFMAs found  {name[:110]}"
    ins = [r[1] for r in loop]
    dma = [i for i, l in enumerate(ins) if l.startswith("buffer_load") and l.rstrip().endswith("lds")]
    if not dma:
        return False, f"FAIL no LDS-DMA issue in the chunk loop  {name[:110]}"
    ins = ins[dma[0]:] + ins[:dma[0]]   # the iteration in the order it runs, from the issue of the next chunk's loads
    last_read = max(i for i, l in enumerate(ins) if l.startswith("ds_read"))
    waits = [i for i, l in enumerate(ins) if l.startswith("s_waitcnt") and "vmcnt" in l]
    early = [i for i in waits if i < last_read]
    scratch = [l for l in ins if l.startswith("scratch_")]
    r = check(name, body)
    m0_ok = r is not None and "foreign M0 writes 0" in r[1]
    ok = len(waits) >= 1 and not early and not scratch and m0_ok
    return ok, (f"{'ok  ' if ok else 'FAIL'} chunk loop of {len(ins)} instructions: vmcnt waits {len(waits)}, of them between the DMA issue and the last LDS read {len(early)} (want 0), "
                f"scratch ops {len(scratch)}, foreign M0 writes {'0' if m0_ok else '>0'}  {name[:110]}")


def main():
    rc = 0
    for obj in sys.argv[1:]:
        for name, body in kernels(disassemble(obj)):
            if "attn_stream" in name:
                r = check_stream(name, body)
                if r is not None:
                    print(r[1])
                    rc |= 0 if r[0] else 1
                continue
            if "nt_pipe_kernel" not in name and "gemm_bf16_tn_kernel" not in name:
                continue
            r = check(name, body)
            if r is None:
                continue
            print(r[1])
            rc |= 0 if r[0] else 1
    sys.exit(rc)


if __name__ == "__main__":
    main()
