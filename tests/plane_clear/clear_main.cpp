// clear_main.cpp — stand-alone host check of the shadow-plane keep masks (shadow_plane_keep,
// csrc/rt_shadow_table.hpp), built and run by tests/test_plane_clear_host.py against the C oracle
// (oracle/rt_oracle.c).  The random frames, the frame file and the oracle's shadow rays are
// tests/host_frame.hpp's.
//
//   clear_main prop SEED CASES [MUTANT]
//       For every tile with an entry (empty cone mask, every plane decided), every lane pixel of
//       it (clamped into the image as the kernel clamps), every light and every shadow ray the
//       oracle casts from a plane: each plane the tile's mask drops for that light must leave the
//       packet kernel's plane classification (pk_occlusion_t, pk_uniform_tile) at a `continue`,
//       evaluated here in FP64 on the oracle's origin, direction and maxDist.  Anything else is a
//       violation.  MUTANT: none (default), light (the light's side of the plane alone decides:
//       the ball's side and its margin are ignored).  (A mutant that drops the ball's own plane
//       whatever the bias reports nothing on these frames — the plane is clear in fact at every
//       bias they use — so it is not kept.)
//   clear_main frame FILE
//       one frame of a real scene (shadow_main's file format): the same check and counts, and
//       the workgroups (two waves side by side) whose tiles are all uniform and fully clear.
// Counts: `plane` the uniform tiles that see a plane (the tiles pk_uniform_tile shades), `clear`
// those of them whose masks are 0 for every light, `proven` the (tile, light, plane) triples
// dropped over all tiles with an entry, `rays` the shadow rays checked against a dropped plane.
// Exit status 0 only when every property holds (mutants: always 0, the caller reads
// `violations`).
#include "../host_frame.hpp"

enum ClearMutant { kClrNone, kClrLight };

struct ClearTile {
    bool entry;                        // the tile has a bound: masks mean something
    unsigned long long cls;            // its class (tile_class_word)
    unsigned keep[kShadowTabLights];   // per light
};

static ClearTile clear_tile(const Frame& F, uint32_t x0, uint32_t yl0, ClearMutant mut) {
    const int ns = static_cast<int>(F.sph.size()), np = static_cast<int>(F.pl.size());
    const int nl = static_cast<int>(F.lt.size());
    const double hw = static_cast<double>(F.cam.width) / 2.0,
                 hh = static_cast<double>(F.cam.height) / 2.0, dz = cam_dz(F.cam);
    const ConeRect q = cone_tile_rect(x0, yl0, F.cam.width, F.rp);
    const uint64_t cone = tile_cone_mask(F, x0, yl0);
    ShadowBound<> B;
    B.n = 0;
    B.ok = false;
    if (cone == 0)
        B = shadow_tile_bound(q, hw, hh, F.cam.position, dz, F.planes.data(), np, F.bias);
    ClearTile T{};
    T.entry = B.ok;
    unsigned long long words[kShadowTabLights] = {0, 0, 0, 0};
    for (int l = 0; l < nl; ++l) {
        words[l] = shadow_tile_word(B, F.lt[l].position, F.bias, F.centre.data(), 3,
                                    F.terms.data() + 7, 8, ns);
        const double* L = F.lt[l].position;
        const double* pl = F.planes.data();
        if (mut == kClrLight) {
            T.keep[l] = shadow_plane_keep<kShadowTabPlanes, false>(B, L, pl, np, F.cam.position,
                                                                   F.bias);
        } else {
            T.keep[l] = shadow_plane_keep(B, L, pl, np, F.cam.position, F.bias);
        }
    }
    const std::vector<double> pln = plane_flags(F);
    T.cls = tile_class_word<kShadowTabPlanes>(cone, B, words, nl, pln.data(), np);
    // the packed word gives back what went in
    const unsigned long long w = tile_class_pack(T.cls, T.keep, nl);
    if (tile_class_of(w) != T.cls) std::abort();
    for (int l = 0; l < nl; ++l)
        if (tile_plane_keep(w, l) != T.keep[l]) std::abort();
    return T;
}

// the kernel's classification of plane i for one shadow ray: true when it leaves at a `continue`
static bool plane_leaves(const double* rec, const double* so, const double* L, double max_dist) {
    const double* qp = rec;
    const double* qn = rec + 3;
    const double dn = dot3(qn, L);
    if (!(std::fabs(dn) > 1e-6)) return true;
    const double w[3] = {qp[0] - so[0], qp[1] - so[1], qp[2] - so[2]};
    const double nm = dot3(w, qn);
    const double A = dn > 0.0 ? nm : -nm, B = std::fabs(dn);
    if (A < -1e-300 * B) return true;
    if (A >= max_dist * B * (1.0 + 1e-9)) return true;
    return false;
}

struct ClearTally {
    uint64_t tiles = 0, entries = 0, uniform = 0, plane = 0, clear = 0, workgroups = 0,
             clear_wgs = 0, proven = 0, possible = 0, rays = 0, violations = 0;
};

static void check_clear_frame(const Frame& F, ClearMutant mut, int tag, ClearTally& T) {
    const o_scene sc = F.scene();
    const int np = static_cast<int>(F.pl.size());
    const size_t nl = F.lt.size();
    const uint32_t gx = (F.cam.width + 15) / 16, gy = (F.rp.rows + 7) / 8;
    Shadow S;
    for (uint32_t ty = 0; ty < gy; ++ty)
        for (uint32_t wx = 0; wx < gx; ++wx) {
            ++T.workgroups;
            int clear_uniform = 0;
            for (uint32_t w = 0; w < 2; ++w) {
                const uint32_t x0 = 8 * (2 * wx + w), yl0 = 8 * ty;
                ++T.tiles;
                const ClearTile C = clear_tile(F, x0, yl0, mut);
                if (!C.entry) {
                    for (size_t k = 0; k < nl; ++k)
                        if (C.keep[k] != kPlaneKeepAll) std::abort();  // no bound, nothing proven
                    continue;
                }
                ++T.entries;
                unsigned any = 0;
                for (size_t k = 0; k < nl; ++k) {
                    any |= C.keep[k];
                    T.possible += static_cast<uint64_t>(np);
                    T.proven += static_cast<uint64_t>(
                        np - __builtin_popcount(C.keep[k] & ((1u << np) - 1u)));
                }
                if (C.cls != kTileGeneral) {
                    ++T.uniform;
                    if (C.cls != kTileSky) {
                        ++T.plane;
                        T.clear += any == 0;
                    }
                    clear_uniform += C.cls == kTileSky || any == 0;
                }
                for (uint32_t l = 0; l < 64; ++l) {
                    uint32_t x, y;
                    bool valid;
                    lane_pixel(F, x0, yl0, l % 8, l / 8, x, y, valid);
                    pixel_shadow(F, sc, x, y, S);
                    if (S.type != 2) continue;  // a miss casts nothing; a sphere: shadow_main's
                    for (size_t k = 0; k < nl; ++k) {
                        if (!S.cast[k]) continue;
                        bool counted = false;
                        for (int i = 0; i < np; ++i) {
                            if ((C.keep[k] >> i) & 1u) continue;
                            if (!counted) ++T.rays, counted = true;
                            if (plane_leaves(&F.planes[8 * static_cast<size_t>(i)], S.so, S.L[k],
                                             S.max_dist[k]))
                                continue;
                            if (T.violations++ < 10)
                                std::fprintf(stderr,
                                             "case %d: %ux%u tile (%u,%u) pixel (%u,%u) light %zu: "
                                             "dropped plane %d is not clear (mask %02x)\n",
                                             tag, F.cam.width, F.cam.height, x0, yl0, x, y, k, i,
                                             C.keep[k]);
                        }
                    }
                }
            }
            T.clear_wgs += clear_uniform == 2;
        }
}

static void print_clear(const char* what, int cases, const ClearTally& T) {
    std::printf("%s cases %d tiles %" PRIu64 " entries %" PRIu64 " uniform %" PRIu64
                " plane %" PRIu64 " clear %" PRIu64 " workgroups %" PRIu64 " clear_wgs %" PRIu64
                " proven %" PRIu64 " possible %" PRIu64 " rays %" PRIu64 " violations %" PRIu64
                "\n",
                what, cases, T.tiles, T.entries, T.uniform, T.plane, T.clear, T.workgroups,
                T.clear_wgs, T.proven, T.possible, T.rays, T.violations);
}

static int run_clear_prop(uint64_t seed, int cases, ClearMutant mut) {
    Rng R{seed};
    ClearTally T;
    for (int c = 0; c < cases; ++c) {
        const Frame F = random_frame(R);
        check_clear_frame(F, mut, c, T);
    }
    print_clear("prop", cases, T);
    if (mut != kClrNone) return 0;
    return T.violations ? 1 : 0;
}

static int run_clear_frame(const char* path) {
    Frame F{};
    if (const int r = read_frame(path, F)) return r;
    ClearTally T;
    check_clear_frame(F, kClrNone, 0, T);
    print_clear("frame", 1, T);
    return T.violations ? 1 : 0;
}

int main(int argc, char** argv) {
    if ((argc == 4 || argc == 5) && !std::strcmp(argv[1], "prop")) {
        ClearMutant mut = kClrNone;
        if (argc == 5) {
            if (!std::strcmp(argv[4], "light")) mut = kClrLight;
            else if (std::strcmp(argv[4], "none")) return 64;
        }
        return run_clear_prop(std::strtoull(argv[2], nullptr, 0), std::atoi(argv[3]), mut);
    }
    if (argc == 3 && !std::strcmp(argv[1], "frame")) return run_clear_frame(argv[2]);
    std::fprintf(stderr, "usage: clear_main prop SEED CASES [none|light] | clear_main frame FILE\n");
    return 64;
}
