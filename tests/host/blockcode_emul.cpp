// Host emulation of the block-code kernels (no GPU): csrc/blockcode_core.hpp's plan, run staging, syndrome_word() and emit(), walked
// workgroup by workgroup and thread by thread exactly as csrc/blockcode.hip schedules them: every thread's share of the run's 16-byte
// chunks (heads and tails byte by byte), the tables' LDS layout, one lane per block / one wave per block with the 64 lanes' words xor-ed /
// one workgroup per block with the waves' words combined through the LDS words, and the output run's chunks.
//   blockcode_emul n k mode tables.u32 in.u8 out.u8 in_offset out_offset        (blockcode_emul n k: print the plan only)
// mode 0 encode, 1 decode; tables.u32: enc[k], syn[n], trap[k]; in.u8: nblocks * (k | n) bytes 0 / 1; out.u8: the result bytes.
// The input window sits in_offset bytes into an allocation of exactly in_offset + len bytes whose head is 0xFF, the output window
// out_offset bytes into one of exactly out_offset + len bytes whose head is a guard that must survive; every global access is checked
// against its window (exit 7) and the LDS is an allocation of exactly the plan's bytes, so -fsanitize=address sees what the checks
// cannot.  Exit 0 and "form F blocks_per_wg B threads T lds L" on stdout.
// Build: g++ -O1 -std=c++17 -I scikit-dsp-comm_amd/csrc tests/host/blockcode_emul.cpp -o /tmp/blockcode_emul
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "blockcode_core.hpp"

using namespace skdsp::blk;

struct Window {
    const uint8_t *lo, *hi;
    void need(const uint8_t *p, int bytes) const
    {
        if (p < lo || p + bytes > hi) {
            fprintf(stderr, "access of %d bytes at window offset %lld outside [0, %lld)\n", bytes, (long long)(p - lo), (long long)(hi - lo));
            exit(7);
        }
    }
};
struct HostMem {
    Window in, out;
    uint8_t ld8(const uint8_t *g) const { in.need(g, 1); return *g; }
    void st8(uint8_t *g, uint8_t v) const { out.need(g, 1); *g = v; }
    void in16(uint8_t *img, const uint8_t *g) const
    {
        in.need(g, 16);
        if (((uintptr_t)g | (uintptr_t)img) & 15) { fprintf(stderr, "unaligned 16-byte load\n"); exit(8); }
        memcpy(img, g, 16);
    }
    void out16(uint8_t *g, const uint8_t *img) const
    {
        out.need(g, 16);
        if (((uintptr_t)g | (uintptr_t)img) & 15) { fprintf(stderr, "unaligned 16-byte store\n"); exit(8); }
        memcpy(g, img, 16);
    }
};

template <class T> static std::vector<T> read_all(const char *path)
{
    std::vector<T> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(4);
    T b[1024];
    size_t n;
    while ((n = fread(b, sizeof(T), 1024, f)) > 0) v.insert(v.end(), b, b + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 9 && argc != 3) return 2;
    const int n = std::atoi(argv[1]), k = std::atoi(argv[2]);
    Plan p;
    const char *why = plan_make(n, k, &p);
    if (why) {
        fprintf(stderr, "%s\n", why);
        return 5;
    }
    if (argc == 3) {   // the plan only
        printf("form %d blocks_per_wg %d threads %d lds %d\n", p.form, p.blocks_per_wg, p.threads, p.lds_bytes);
        return 0;
    }
    const int mode = std::atoi(argv[3]), in_off = std::atoi(argv[7]), out_off = std::atoi(argv[8]);
    const std::vector<uint32_t> tables = read_all<uint32_t>(argv[4]);
    if ((int)tables.size() != 2 * k + n) return 6;
    const uint32_t *enc = tables.data(), *syn = enc + k, *trap = syn + n;
    if (!tables_fit(p, enc, syn, trap)) return 6;
    const std::vector<uint8_t> bits = read_all<uint8_t>(argv[5]);
    const int nin = bytes_in(p, mode), nout = bytes_out(p, mode);
    if (bits.empty() || bits.size() % nin) return 6;
    const int64_t nblocks = (int64_t)(bits.size() / nin);

    uint8_t *in_buf = new uint8_t[in_off + bits.size()], *out_buf = new uint8_t[out_off + nblocks * nout];
    if (((uintptr_t)in_buf | (uintptr_t)out_buf) & 15) return 9;   // the offsets are meant relative to a 16-byte boundary
    memset(in_buf, 0xFF, in_off);
    memcpy(in_buf + in_off, bits.data(), bits.size());
    memset(out_buf, 0xA5, out_off);
    memset(out_buf + out_off, 0xEE, nblocks * nout);
    HostMem mem;
    mem.in = {in_buf + in_off, in_buf + in_off + bits.size()};
    mem.out = {out_buf + out_off, out_buf + out_off + nblocks * nout};
    const uint32_t *tab = mode == kEncode ? enc : syn;

    const int T = p.threads, W = T / kLanes;
    for (int64_t g = 0; g < grid_of(p, nblocks); ++g) {
        uint8_t *lds = new uint8_t[p.lds_bytes];
        if ((uintptr_t)lds & 15) return 9;
        memset(lds, 0xCD, p.lds_bytes);   // nothing may depend on what the LDS held
        uint8_t *img_in = lds + p.off_in, *img_out = lds + p.off_out;
        uint32_t *tab_lds = reinterpret_cast<uint32_t *>(lds + p.off_tab), *trap_lds = reinterpret_cast<uint32_t *>(lds + p.off_trap);
        uint32_t *red = reinterpret_cast<uint32_t *>(lds + p.off_red);
        const int nb = blocks_of(p, nblocks, g);
        const uint8_t *gin = mem.in.lo + g * p.blocks_per_wg * nin;
        uint8_t *gout = const_cast<uint8_t *>(mem.out.lo) + g * p.blocks_per_wg * nout;
        for (int t = 0; t < T; ++t) {
            stage_in(mem, gin, nb * nin, img_in, t, T);
            if (p.form != kGroup) {
                for (int i = t; i < nin; i += T) tab_lds[tab_index(p, i)] = tab[i];
                if (mode == kDecode)
                    for (int i = t; i < p.k; i += T) trap_lds[i] = trap[i];
            }
        }
        // ---- barrier
        const int s0 = lead_of(gin), o0 = lead_of(gout);
        if (p.form == kLane) {
            for (int t = 0; t < T && t < nb; ++t) {
                const int s = s0 + t * nin, o = o0 + t * nout;
                const uint32_t w = syndrome_word(p, img_in, s, nin, tab_lds, 0, 1);
                for (int i = 0; i < nout; ++i)
                    img_out[o + i] = emit(p, mode, i, i < p.k ? img_in[s + i] : (uint8_t)0, w, mode == kDecode ? trap_lds[i] : 0u);
            }
        } else if (p.form == kWave) {
            for (int wave = 0; wave < W; ++wave)
                for (int b = wave; b < nb; b += W) {
                    const int s = s0 + b * nin, o = o0 + b * nout;
                    uint32_t w = 0;
                    for (int lane = 0; lane < kLanes; ++lane) w ^= syndrome_word(p, img_in, s, nin, tab_lds, lane, kLanes);   // the butterfly's result in every lane
                    for (int lane = 0; lane < kLanes; ++lane)
                        for (int i = lane; i < nout; i += kLanes)
                            img_out[o + i] = emit(p, mode, i, i < p.k ? img_in[s + i] : (uint8_t)0, w, mode == kDecode ? trap_lds[i] : 0u);
                }
        } else {
            for (int wave = 0; wave < W; ++wave) {
                uint32_t w = 0;
                for (int lane = 0; lane < kLanes; ++lane) w ^= syndrome_word(p, img_in, s0, nin, tab, wave * kLanes + lane, T);
                red[wave] = w;
            }
            // ---- barrier
            uint32_t w = 0;
            for (int v = 0; v < W; ++v) w ^= red[v];
            for (int t = 0; t < T; ++t)
                for (int i = t; i < nout; i += T)
                    img_out[o0 + i] = emit(p, mode, i, i < p.k ? img_in[s0 + i] : (uint8_t)0, w, mode == kDecode ? trap[i] : 0u);
        }
        // ---- barrier
        for (int t = 0; t < T; ++t) stage_out(mem, gout, nb * nout, img_out, t, T);
        delete[] lds;
    }
    for (int i = 0; i < out_off; ++i)
        if (out_buf[i] != 0xA5) {
            fprintf(stderr, "guard byte %d in front of the output window was overwritten\n", i);
            return 7;
        }
    FILE *f = fopen(argv[6], "wb");
    if (!f) return 4;
    fwrite(out_buf + out_off, 1, (size_t)(nblocks * nout), f);
    fclose(f);
    printf("form %d blocks_per_wg %d threads %d lds %d\n", p.form, p.blocks_per_wg, p.threads, p.lds_bytes);
    delete[] in_buf;
    delete[] out_buf;
    return 0;
}
