"""Instruction mix of one kernel from hipcc's --save-temps assembly: python tools/isa_count.py <file.s> [--loop] <kernel name substring> ...
--loop counts only the kernel's largest outermost (depth-1) loop that loads from global memory (any loop if none does): every block the
compiler's comments place in that loop, inner loops, cold paths and the header block included.  This is the tool's own definition of "the
loop"; a count of a hand-picked hot region (such as the 8246 instructions quoted when the LDS stage was proposed) covers less."""
import re
import sys
from collections import Counter
LABEL = re.compile(r"BB[0-9]+_[0-9]+")          # a basic-block label inside one of the compiler's loop comments
norm = lambda label: label.lstrip(".").removeprefix("L")      # .LBB12_15 (a label) and BB12_15 (in a comment) name one block
loop = "--loop" in sys.argv
args = [a for a in sys.argv[1:] if a != "--loop"]
s = open(args[0]).read()
for want in args[1:]:
    for line in s.splitlines():
        if want in line and not line.startswith((".", "\t", " ")) and ":" in line and line.split(":")[0].strip().isidentifier():
            k = line.split(":")[0]
            i = s.index("\n" + k + ":")
            j = s.find(".Lfunc_end", i)
            body = s[i:j if j > 0 else len(s)]
            if loop:
                # the blocks of the kernel's largest outermost loop (the compiler's own "in Loop: Header=... Depth=..." block comments,
                # inner loops included), the header block with them
                blocks, cur = {}, None
                for l in body.splitlines():
                    if l and not l.startswith(("\t", " ", ";")) and ":" in l:
                        cur = l.split(":")[0]; blocks[cur] = {"lines": [], "hdr": None, "depth": 0}
                    elif cur:
                        if "Loop Header: Depth=1" in l: blocks[cur]["hdr"] = cur
                        elif ("in Loop: Header=" in l or "Parent Loop " in l) and "Depth=1" in l:
                            m = LABEL.search(l.split("Header=" if "Header=" in l else "Parent Loop ")[1])
                            if m: blocks[cur]["hdr"] = m.group(0)
                        blocks[cur]["lines"].append(l)
                sizes = Counter()
                for b in blocks.values():
                    if b["hdr"]: sizes[norm(b["hdr"])] += sum(1 for l in b["lines"] if l.startswith("\t") and not l.strip().startswith((".", ";")))
                gathers = {norm(b["hdr"]) for b in blocks.values() if b["hdr"] and any(l.startswith("\tglobal_load") for l in b["lines"])}
                hdr = next((h for h, _ in sizes.most_common() if h in gathers or not gathers), None)
                if hdr is None:
                    print(k[:60], "has no depth-1 loop (no 'Loop Header: Depth=1' comment in its assembly): nothing to count with --loop")
                    break
                body = "\n".join("\n".join(b["lines"]) for b in blocks.values() if b["hdr"] and norm(b["hdr"]) == hdr)
                k += " loop " + hdr
            ins = [l.split()[0] for l in body.splitlines() if l.startswith("\t") and l.strip() and not l.strip().startswith((".", ";"))]
            c = Counter(ins)
            top = ("v_mad_u64_u32", "v_mul_lo_u32", "v_addc_co_u32_e32", "v_addc_co_u32_e64", "ds_read_b64", "ds_read2_b64", "ds_read_b128", "ds_write_b64", "ds_write2_b64", "ds_read_b32", "ds_write_b32",
                   "s_waitcnt", "s_barrier", "v_cndmask_b32_e32", "global_load_lds_dwordx4", "global_load_dwordx4", "global_store_dwordx4", "scratch_load_dword", "scratch_store_dword", "v_mov_b32_e32", "v_mov_b64_e32", "s_nop")
            print(k[:60], "total", len(ins), {x: c[x] for x in top if c[x]})
            break
