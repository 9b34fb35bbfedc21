"""The global-memory requests of one kernel's tile loop and the address arithmetic around them: per basic block that holds a global_load /
global_store, the number of requests (and how many of them take their base from an SGPR pair, the `saddr` form), of vector integer adds
(v_add_co_u32 / v_addc_co_u32 / v_add_u32 / v_lshl_add_u64 ... -- what forms a 64-bit lane address), of scalar adds and of s_nop, then the totals
of the loop with its packed and scalar float instructions.
    hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -Iinclude csrc/fir_ols.hip -o fir_ols.s
    python tools/ols_vmem_addr.py fir_ols.s 'ols_tile_kernel<false, false, false, false>' [--min-requests N | --all-blocks]
(--min-requests 8: only the whole-tile copies, not the one-request blocks of the element-wise edge paths)
The tile loop is the longest backward branch of the function (tools/ols_lds_chain.py); blocks in layout order."""
import os, re, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ols_lds_chain import function_lines, tile_loop

VADD = re.compile(r"^v_(add_co_u32|addc_co_u32|add_u32|add3_u32|add_lshl_u32|lshl_add_u32|lshl_add_u64|lshlrev_b64|mad_u64_u32|mad_i64_i32|ashrrev_i64)")
SADD = re.compile(r"^s_(add_u32|addc_u32|add_i32|lshl_b64)")
FSCALAR = re.compile(r"^v_(mul_f32|fma_f32|fmac_f32|fmamk_f32|fmaak_f32|add_f32|sub_f32)")
KEYS = ("global_load", "global_store", "saddr", "vec_int_add", "scalar_add", "s_nop", "nop_states")

def count(lines):
    c = dict.fromkeys(KEYS + ("valu", "v_pk", "v_f32_scalar", "v_readlane"), 0)
    for l in lines:
        s = l.strip()
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        if op.startswith(("global_load", "global_store")):
            c["global_load" if op.startswith("global_load") else "global_store"] += 1
            if re.search(r"\bs\[\d+:\d+\]", s): c["saddr"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1; c["nop_states"] += int(s.split()[1]) + 1
        elif SADD.match(op):
            c["scalar_add"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if VADD.match(op): c["vec_int_add"] += 1
            elif op.startswith("v_pk_"): c["v_pk"] += 1
            elif FSCALAR.match(op): c["v_f32_scalar"] += 1
            elif op.startswith("v_readlane"): c["v_readlane"] += 1
    return c

def main():
    path, want = sys.argv[1], sys.argv[2]
    name, body = function_lines(path, want)
    loop = tile_loop(body)
    blocks, cur = [], ["(loop head)", []]
    for l in loop:
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            blocks.append(cur); cur = [m.group(1), []]
        else:
            cur[1].append(l)
    blocks.append(cur)
    least = int(sys.argv[sys.argv.index("--min-requests") + 1]) if "--min-requests" in sys.argv else 1
    print(name, "tile loop: %d lines, %d blocks" % (len(loop), len(blocks)))
    for label, lines in blocks:
        c = count(lines)
        if c["global_load"] + c["global_store"] >= least or "--all-blocks" in sys.argv:
            print("  %-12s %s" % (label, " ".join("%s=%d" % (k, c[k]) for k in KEYS)))
    c = count(loop)
    print("loop: " + " ".join("%s=%d" % kv for kv in c.items()))
    print("function: v_readlane=%d" % count(body)["v_readlane"])

if __name__ == "__main__":
    main()
