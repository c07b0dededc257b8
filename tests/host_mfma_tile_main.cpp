// Stand-alone play of the dense tile of csrc/ebm_mfma_tile.h for tests/test_host_mfma_tile.py: no HIP, no GPU; only the
// constexpr part of the header is seen here.
//   coverage            the D map over 256 lanes x 2 x 2 accumulators x 4 registers: how many cells of the 64 x 64 tile are hit
//                       exactly once
//   play [f32-rows]     one workgroup: both sides filled with small distinct integers, in a line-major and in a k-major LDS image
//                       (the padding poisoned); every lane's operands taken through the header's operand map and accessors; the
//                       instruction applied as the header's comment states it, restated below from that sentence and not from
//                       the header's functions; the results collected through the D map and compared with the plain triple
//                       loop, for 1, 2, 3 and 4 groups issued.  One line per layout and group count with the number of wrong
//                       cells.  f32-rows: the control — the instruction's D restated with the row formula of the f32
//                       instructions, (l >> 4) * 4 + g, which must come out wrong.
// Exit status 1 if anything is wrong.
#include <cstdio>
#include <cstring>

#include "../energybalancemodel.jl_amd/csrc/ebm_mfma_tile.h"

using namespace ebm;

namespace {

constexpr double kPoison = -7777.0;
long long a_value(int line, int k) { return 1 + line * kTileChunk + k; }                   // 1 ... 1024, all distinct
long long b_value(int line, int k) { return 2000 + 17 * (line * kTileChunk + k); }         // distinct, and no multiple of A's

// v_mfma_f64_16x16x4_f64 as the header states it: D[i][j] += sum_k A[i][k] * B[j][k]; lane l supplies A[l & 15][l >> 4] and
// B[l & 15][l >> 4]; register g of lane l is D[(l >> 4) + 4 g][l & 15].  a, b: the 64 lanes' operands; d: their 4 registers.
void mfma(const double (&a)[64], const double (&b)[64], double (&d)[64][4], bool f32_rows) {
    double A[16][4], B[16][4];
    for (int l = 0; l < 64; ++l) {
        A[l & 15][l >> 4] = a[l];
        B[l & 15][l >> 4] = b[l];
    }
    for (int l = 0; l < 64; ++l)
        for (int g = 0; g < 4; ++g) {
            const int i = f32_rows ? (l >> 4) * 4 + g : (l >> 4) + 4 * g, j = l & 15;
            for (int k = 0; k < 4; ++k) d[l][g] += A[i][k] * B[j][k];
        }
}

template <class SIDE>
int play(const SIDE *sa, const SIDE *sb, int groups, bool f32_rows) {
    static double acc[kTileLanes][2][2][4];
    std::memset(acc, 0, sizeof(acc));
    for (int wave = 0; wave < kTileLanes / 64; ++wave)
        for (int n = 0; n < groups; ++n)
            for (int s = 0; s < 2; ++s)
                for (int t = 0; t < 2; ++t) {
                    double a[64], b[64], d[64][4];
                    for (int l = 0; l < 64; ++l) {
                        const int tid = 64 * wave + l;
                        const TileOperand oa = tile_operand_a(tid, s), ob = tile_operand_b(tid, t);
                        a[l] = tile_lds(sa, oa.line, 4 * n + oa.k);
                        b[l] = tile_lds(sb, ob.line, 4 * n + ob.k);
                        for (int g = 0; g < 4; ++g) d[l][g] = acc[tid][s][t][g];
                    }
                    mfma(a, b, d, f32_rows);
                    for (int l = 0; l < 64; ++l)
                        for (int g = 0; g < 4; ++g) acc[64 * wave + l][s][t][g] = d[l][g];
                }
    static double got[kTileSide][kTileSide];
    static int written[kTileSide][kTileSide];
    std::memset(written, 0, sizeof(written));
    for (int tid = 0; tid < kTileLanes; ++tid)
        for (int s = 0; s < 2; ++s)
            for (int t = 0; t < 2; ++t)
                for (int g = 0; g < 4; ++g) {
                    const TileCell c = tile_cell(tid, s, t, g);
                    if (c.row < 0 || c.row >= kTileSide || c.col < 0 || c.col >= kTileSide) return kTileSide * kTileSide;
                    got[c.row][c.col] = acc[tid][s][t][g];
                    ++written[c.row][c.col];
                }
    int wrong = 0;
    for (int r = 0; r < kTileSide; ++r)
        for (int c = 0; c < kTileSide; ++c) {
            long long want = 0;
            for (int k = 0; k < 4 * groups; ++k) want += a_value(r, k) * b_value(c, k);
            wrong += written[r][c] != 1 || got[r][c] != (double)want;
        }
    return wrong;
}

int coverage() {
    static int hits[kTileSide][kTileSide];
    int outside = 0, once = 0;
    for (int tid = 0; tid < kTileLanes; ++tid)
        for (int s = 0; s < 2; ++s)
            for (int t = 0; t < 2; ++t)
                for (int g = 0; g < 4; ++g) {
                    const TileCell c = tile_cell(tid, s, t, g);
                    if (c.row < 0 || c.row >= kTileSide || c.col < 0 || c.col >= kTileSide) ++outside;
                    else ++hits[c.row][c.col];
                }
    for (auto &row : hits)
        for (int h : row) once += h == 1;
    std::printf("coverage results %d outside %d cells %d once %d\n", kTileLanes * 16, outside, kTileSide * kTileSide, once);
    return outside == 0 && once == kTileSide * kTileSide ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "coverage")) return coverage();
    if (argc >= 2 && !std::strcmp(argv[1], "play")) {
        const bool f32_rows = argc == 3 && !std::strcmp(argv[2], "f32-rows");
        if (argc > 2 && !f32_rows) return 2;
        static tile_line_major la[kTileSide], lb[kTileSide];
        static tile_k_major ka[kTileChunk], kb[kTileChunk];
        for (auto &row : la) for (double &x : row) x = kPoison;
        for (auto &row : lb) for (double &x : row) x = kPoison;
        for (auto &row : ka) for (double &x : row) x = kPoison;
        for (auto &row : kb) for (double &x : row) x = kPoison;
        for (int line = 0; line < kTileSide; ++line)
            for (int k = 0; k < kTileChunk; ++k) {
                la[line][k] = ka[k][line] = (double)a_value(line, k);
                lb[line][k] = kb[k][line] = (double)b_value(line, k);
            }
        int bad = 0;
        for (int groups = 1; groups <= kTileChunk / 4; ++groups) {
            const int wl = play(la, lb, groups, f32_rows), wk = play(ka, kb, groups, f32_rows);
            std::printf("play line-major groups %d wrong %d\nplay k-major groups %d wrong %d\n", groups, wl, groups, wk);
            bad += (wl != 0) + (wk != 0);
        }
        return bad ? 1 : 0;
    }
    std::fprintf(stderr, "usage: %s coverage | play [f32-rows]\n", argv[0]);
    return 2;
}
