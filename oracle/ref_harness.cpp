// oracle/ref_harness.cpp — TEST INFRASTRUCTURE ONLY.
//
// Drives the UNMODIFIED reference renderer (compiled by oracle/Makefile from
// /root/reference/RaytracingEngine/*.{h,cpp} where they lie) so its outputs can pin the C
// restatement in oracle/rt_oracle.c and serve as the "reference" CPU baseline.  Nothing here
// re-implements reference behaviour: it parses a scene file, builds reference objects through
// the reference's public API and calls it.
//
// Modes (all binary files are little-endian float64 unless noted):
//   render  <scene.txt> <out.f64|-> [repeat]  Scene::RenderImage(); prints {"ms":[...]} per run
//   tonemap <in.f64> <n> <out.u8>             tonemapAll() (7 ops) then tonemap() → 8*n*3 bytes
//   curves  <in.f64> <n> <out.f64>            the 7 operator curves before toColor → 7*n*3
//   kat     sphere|plane|triangle|getray <in.f64> <n> <out.f64>
//   closest <scene.txt> <rays.f64> <n> <out.f64>   IntersectClosest → n*9 doubles
//   trace   <scene.txt> <rays.f64> <n> <bias> <out.f64> [max_recursion]
//                                             Scene::TraceRay(ray, 0, bias) → n*3, with
//                                             scene.maxRecursion set when given (default 10)
//   anybefore <scene.txt> <rays.f64> <dist.f64> <n> <out.u8>
//                                             Scene::IntersectAnyBefore(ray, maxDist) → n bytes 0/1
//   transmit <scene.txt> <rays.f64> <dist.f64> <n> <bias> <out.f64>
//                                             Scene::computeTransmittance(ray, maxDist, bias) → n
//   direct  <scene.txt> <points.f64 n*9> <materials.f64 n*7> <n> <bias> <out.f64 n*9> [light]
//                                             Scene::directLightning three times per point
//                                             {p, normal, view}: → {radiance, diffuse accumulator,
//                                             specular accumulator}; with `light`, the scene is
//                                             built with that one light only
//   ppm     <in.u8> <w> <h> <out.ppm>         writePPM()
//   version                                   prints the SHA-256 prefix of this file the binary
//                                             was built from (oracle/Makefile rebuilds on a mismatch)
// The standard headers come first so that only the reference's own classes are seen with
// `private` spelled `public` below: mode `trace` calls Scene::TraceRay, a private member of the
// reference's Scene (Scene.h:131), `transmit` Scene::computeTransmittance (Scene.h:35) and `direct`
// Scene::directLightning (Scene.h:79).  The reference's sources are read where they lie, unedited.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <optional>
#include <random>
#include <ranges>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#ifdef _OPENMP
#include <omp.h>
#endif

#define private public
#include "Math.h"
#include "Shape.h"
#include "Light.h"
#include "Scene.h"
#undef private
#include "Image.h"

// Free functions defined in /root/reference/RaytracingEngine/RaytracingEngine.cpp (linked
// from that translation unit, compiled with its main() renamed away).
std::vector<Color> tonemap(const std::vector<Vec3>& pixels);
std::vector<std::vector<Color>> tonemapAll(const std::vector<Vec3> pixels);
Vec3 simple(const Vec3& color);
Vec3 reinhardSimple(const Vec3& color);
Vec3 reinhardExtended(const Vec3 color, double max_white);
Vec3 reinhardExtendedLuminance(const Vec3& color, double maxWhite);
Vec3 reinhardJodie(const Vec3& color, double a);
Vec3 uncharted2(const Vec3& color);
Vec3 aces_approx(Vec3 v);

// defined by the reference application file (compiled with main renamed, oracle/Makefile)
Model LoadObject(const std::string& modelName, const Transform& transform,
                 const Material& material);

namespace {

std::vector<double> read_f64(const char* path, size_t count) {
    std::vector<double> v(count);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(double), count, f) != count) {
        std::fprintf(stderr, "cannot read %zu doubles from %s\n", count, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

void write_bytes(const char* path, const void* p, size_t n) {
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) {
        std::fprintf(stderr, "cannot write %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
}

Material read_material(std::istringstream& in) {
    Material m;
    in >> m.color.x >> m.color.y >> m.color.z >> m.shininess >> m.specular >> m.transparency >>
        m.refractiveIndex;
    return m;
}

Vec3 read_vec(std::istringstream& in) {
    Vec3 v;
    in >> v.x >> v.y >> v.z;
    return v;
}

struct Loaded {
    Camera camera{Vec3(0, 0, 0)};
    std::vector<Sphere> spheres;
    std::vector<Plane> planes;
    std::vector<Triangle> triangles;
    std::vector<Model> models;
    std::vector<Light> lights;
};

// Scene file format: see raytracingengine_amd/scenefile.py (writer) — one record per line.
Loaded load_scene(const char* path) {
    std::ifstream f(path);
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    Loaded L;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string tag;
        in >> tag;
        if (tag == "camera") {
            Vec3 pos = read_vec(in);
            double focal, near_d, far_d;
            size_t w, h;
            int aa;
            in >> focal >> w >> h >> near_d >> far_d >> aa;
            L.camera = Camera(pos, focal, w, h, near_d, far_d);
            L.camera.antiAliasingAmount = aa;
        } else if (tag == "sphere") {
            Vec3 c = read_vec(in);
            double r;
            in >> r;
            Material m = read_material(in);
            L.spheres.emplace_back(r, c, m);
        } else if (tag == "plane") {
            Vec3 p = read_vec(in);
            Vec3 n = read_vec(in);
            Material m = read_material(in);
            L.planes.emplace_back(p, n, m);
        } else if (tag == "triangle") {
            Vec3 a = read_vec(in), b = read_vec(in), c = read_vec(in), t = read_vec(in);
            Material m = read_material(in);
            Transform tf{t, Vec3(0, 0, 0), Vec3(1, 1, 1)};
            L.triangles.emplace_back(a, b, c, m, tf);
        } else if (tag == "model") {
            size_t n;
            in >> n;
            Vec3 t = read_vec(in);
            Material m = read_material(in);
            std::vector<Vec3> pos;
            std::vector<int> idx;
            for (size_t i = 0; i < n; ++i) {
                std::getline(f, line);
                std::istringstream vin(line);
                std::string vtag;
                vin >> vtag;
                for (int k = 0; k < 3; ++k) {
                    pos.push_back(read_vec(vin));
                    idx.push_back(static_cast<int>(pos.size() - 1));
                }
            }
            Transform tf{t, Vec3(0, 0, 0), Vec3(1, 1, 1)};
            L.models.emplace_back(idx, tf, m, pos);
        } else if (tag == "light") {
            Vec3 p = read_vec(in), c = read_vec(in);
            double inten;
            in >> inten;
            L.lights.emplace_back(p, c, inten);
        }
    }
    return L;
}

// only_light >= 0: the scene gets that one light of the file and no other.
Scene build_scene(Loaded& L, long only_light = -1) {
    Scene s(L.camera);
    for (auto& x : L.spheres) s.AddSphere(x);
    for (auto& x : L.planes) s.AddPlane(x);
    for (auto& x : L.triangles) s.AddTriangle(x);
    for (auto& x : L.models) s.AddModel(x);
    for (size_t i = 0; i < L.lights.size(); ++i)
        if (only_light < 0 || static_cast<size_t>(only_light) == i) s.AddLight(L.lights[i]);
    return s;
}

int mode_render(int argc, char** argv) {
    if (argc < 4) return 1;
    Loaded L = load_scene(argv[2]);
    Scene scene = build_scene(L);
    int repeat = argc > 4 ? std::atoi(argv[4]) : 1;
    std::vector<Vec3> px;
    std::printf("{\"threads\": %d, \"ms\": [",
#ifdef _OPENMP
                omp_get_max_threads()
#else
                1
#endif
    );
    for (int r = 0; r < repeat; ++r) {
        auto t0 = std::chrono::steady_clock::now();
        px = scene.RenderImage();
        auto t1 = std::chrono::steady_clock::now();
        std::printf("%s%.3f", r ? ", " : "",
                    std::chrono::duration<double, std::milli>(t1 - t0).count());
        std::fflush(stdout);
    }
    std::printf("]}\n");
    if (std::strcmp(argv[3], "-") != 0)
        write_bytes(argv[3], px.data(), px.size() * sizeof(Vec3));
    return 0;
}

std::vector<Vec3> to_vec3(const std::vector<double>& d) {
    std::vector<Vec3> v(d.size() / 3);
    for (size_t i = 0; i < v.size(); ++i) v[i] = Vec3(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    return v;
}

int mode_tonemap(int argc, char** argv) {
    if (argc < 5) return 1;
    size_t n = std::strtoull(argv[3], nullptr, 10);
    auto px = to_vec3(read_f64(argv[2], 3 * n));
    auto all = tonemapAll(px);
    all.push_back(tonemap(px));
    std::vector<uint8_t> out;
    for (auto& img : all)
        for (auto& c : img) {
            out.push_back(c.r);
            out.push_back(c.g);
            out.push_back(c.b);
        }
    write_bytes(argv[4], out.data(), out.size());
    return 0;
}

int mode_curves(int argc, char** argv) {
    if (argc < 5) return 1;
    size_t n = std::strtoull(argv[3], nullptr, 10);
    auto px = to_vec3(read_f64(argv[2], 3 * n));
    std::vector<double> out;
    auto push = [&](const Vec3& v) {
        out.push_back(v.x);
        out.push_back(v.y);
        out.push_back(v.z);
    };
    for (int op = 0; op < 7; ++op)
        for (auto& c : px) {
            switch (op) {
            case 0: push(simple(c)); break;
            case 1: push(reinhardSimple(c)); break;
            case 2: push(reinhardExtended(c, 5.0)); break;
            case 3: push(reinhardExtendedLuminance(c, 5.0)); break;
            case 4: push(reinhardJodie(c, 0.18)); break;
            case 5: push(uncharted2(c)); break;
            default: push(aces_approx(c)); break;
            }
        }
    write_bytes(argv[4], out.data(), out.size() * sizeof(double));
    return 0;
}

int mode_kat(int argc, char** argv) {
    if (argc < 6) return 1;
    std::string kind = argv[2];
    size_t n = std::strtoull(argv[4], nullptr, 10);
    size_t rec = kind == "sphere" ? 10 : kind == "plane" ? 12 : kind == "triangle" ? 18 : 8;
    auto in = read_f64(argv[3], rec * n);
    std::vector<double> out;
    for (size_t i = 0; i < n; ++i) {
        const double* r = &in[rec * i];
        Rayon ray(Vec3(r[0], r[1], r[2]), Vec3(r[3], r[4], r[5]));
        if (kind == "sphere") {
            Sphere s(r[9], Vec3(r[6], r[7], r[8]));
            auto t = s.Intersect(ray);
            out.push_back(t ? 1.0 : 0.0);
            out.push_back(t ? *t : 0.0);
        } else if (kind == "plane") {
            Plane p(Vec3(r[6], r[7], r[8]), Vec3(r[9], r[10], r[11]));
            auto t = p.Intersect(ray);
            Vec3 nn = p.GetNormal();
            out.push_back(t ? 1.0 : 0.0);
            out.push_back(t ? *t : 0.0);
            out.push_back(nn.x);
            out.push_back(nn.y);
            out.push_back(nn.z);
        } else if (kind == "triangle") {
            Transform tf{Vec3(r[15], r[16], r[17]), Vec3(0, 0, 0), Vec3(1, 1, 1)};
            Triangle tr(Vec3(r[6], r[7], r[8]), Vec3(r[9], r[10], r[11]),
                        Vec3(r[12], r[13], r[14]), Material(), tf);
            auto t = tr.Intersect(ray);
            Vec3 nn = tr.GetNormalAt().value();
            out.push_back(t ? 1.0 : 0.0);
            out.push_back(t ? *t : 0.0);
            out.push_back(nn.x);
            out.push_back(nn.y);
            out.push_back(nn.z);
        } else {  // getray: {px,py,pz,focal,W,H,x,y} — no jitter (aa=false)
            Camera cam(Vec3(r[0], r[1], r[2]), r[3], static_cast<size_t>(r[4]),
                       static_cast<size_t>(r[5]), 0.0, 200.0);
            Rayon g = cam.getRay(static_cast<size_t>(r[6]), static_cast<size_t>(r[7]), false);
            for (double v : {g.origin.x, g.origin.y, g.origin.z, g.direction.x, g.direction.y,
                             g.direction.z})
                out.push_back(v);
        }
    }
    write_bytes(argv[5], out.data(), out.size() * sizeof(double));
    return 0;
}

int mode_closest(int argc, char** argv) {
    if (argc < 6) return 1;
    Loaded L = load_scene(argv[2]);
    Scene scene = build_scene(L);
    size_t n = std::strtoull(argv[4], nullptr, 10);
    auto rays = read_f64(argv[3], 6 * n);
    std::vector<double> out;
    for (size_t i = 0; i < n; ++i) {
        const double* r = &rays[6 * i];
        Rayon ray(Vec3(r[0], r[1], r[2]), Vec3(r[3], r[4], r[5]));
        auto h = scene.IntersectClosest(ray);
        if (!h) {
            for (int k = 0; k < 9; ++k) out.push_back(k == 1 ? -1.0 : 0.0);
            continue;
        }
        out.push_back(static_cast<double>(static_cast<int>(h->type)));
        out.push_back(static_cast<double>(h->index));
        out.push_back(h->distance);
        out.push_back(h->normal.x);
        out.push_back(h->normal.y);
        out.push_back(h->normal.z);
        out.push_back(h->hitPoint.x);
        out.push_back(h->hitPoint.y);
        out.push_back(h->hitPoint.z);
    }
    write_bytes(argv[5], out.data(), out.size() * sizeof(double));
    return 0;
}

// Scene::TraceRay(Rayon, 0, bias) per ray (GenerateAntiAliasing's body, Scene.h:306-309, on a
// caller-given ray instead of camera.getRay's).
int mode_trace(int argc, char** argv) {
    if (argc < 7) return 1;
    Loaded L = load_scene(argv[2]);
    Scene scene = build_scene(L);
    if (argc > 7) scene.maxRecursion = std::atoi(argv[7]);
    size_t n = std::strtoull(argv[4], nullptr, 10);
    const double bias = std::strtod(argv[5], nullptr);
    auto rays = read_f64(argv[3], 6 * n);
    std::vector<double> out;
    for (size_t i = 0; i < n; ++i) {
        const double* r = &rays[6 * i];
        Rayon ray(Vec3(r[0], r[1], r[2]), Vec3(r[3], r[4], r[5]));
        const Vec3 c = scene.TraceRay(ray, 0, bias).value();
        out.push_back(c.x);
        out.push_back(c.y);
        out.push_back(c.z);
    }
    write_bytes(argv[6], out.data(), out.size() * sizeof(double));
    return 0;
}

// Scene::IntersectAnyBefore(ray, maxDist) per ray and distance: one byte each, 0 or 1.
int mode_anybefore(int argc, char** argv) {
    if (argc < 7) return 1;
    Loaded L = load_scene(argv[2]);
    Scene scene = build_scene(L);
    size_t n = std::strtoull(argv[5], nullptr, 10);
    auto rays = read_f64(argv[3], 6 * n);
    auto dist = read_f64(argv[4], n);
    std::vector<uint8_t> out(n);
    for (size_t i = 0; i < n; ++i) {
        const double* r = &rays[6 * i];
        Rayon ray(Vec3(r[0], r[1], r[2]), Vec3(r[3], r[4], r[5]));
        out[i] = scene.IntersectAnyBefore(ray, dist[i]) ? 1 : 0;
    }
    write_bytes(argv[6], out.data(), out.size());
    return 0;
}

// Scene::computeTransmittance(ray, maxDist, bias) per ray and distance.
int mode_transmit(int argc, char** argv) {
    if (argc < 8) return 1;
    Loaded L = load_scene(argv[2]);
    Scene scene = build_scene(L);
    size_t n = std::strtoull(argv[5], nullptr, 10);
    const double bias = std::strtod(argv[6], nullptr);
    auto rays = read_f64(argv[3], 6 * n);
    auto dist = read_f64(argv[4], n);
    std::vector<double> out(n);
    for (size_t i = 0; i < n; ++i) {
        const double* r = &rays[6 * i];
        Rayon ray(Vec3(r[0], r[1], r[2]), Vec3(r[3], r[4], r[5]));
        out[i] = scene.computeTransmittance(ray, dist[i], bias);
    }
    write_bytes(argv[7], out.data(), out.size() * sizeof(double));
    return 0;
}

// Scene::directLightning(HitInfo{hitPoint, material}, viewDir, normal, bias) per point
// {p, normal, view} and material {colour, shininess, specular, transparency, refractiveIndex}.
// The function returns colour * diffuseAccumulation + specularAccumulation * specular
// (Scene.h:126-128), so its two accumulators are read through two more calls with other
// materials: colour (1,1,1) and specular 0 closes the specular branch (Scene.h:115) and returns
// the diffuse accumulator; colour (0,0,0) and specular 1, transparency and shininess unchanged,
// returns the specular accumulator (0 * diffuseAccumulation is NaN where that is not finite).
// Where the point's own specular is not > 0 the branch is closed for it: written as zero.
int mode_direct(int argc, char** argv) {
    if (argc < 8) return 1;
    Loaded L = load_scene(argv[2]);
    Scene scene = build_scene(L, argc > 8 ? std::atol(argv[8]) : -1);
    size_t n = std::strtoull(argv[5], nullptr, 10);
    const double bias = std::strtod(argv[6], nullptr);
    auto pts = read_f64(argv[3], 9 * n);
    auto mats = read_f64(argv[4], 7 * n);
    std::vector<double> out;
    auto push = [&](const Vec3& v) {
        out.push_back(v.x);
        out.push_back(v.y);
        out.push_back(v.z);
    };
    for (size_t i = 0; i < n; ++i) {
        const double* p = &pts[9 * i];
        const double* m = &mats[7 * i];
        const Vec3 normal(p[3], p[4], p[5]), view(p[6], p[7], p[8]);
        Material own;
        own.color = Vec3(m[0], m[1], m[2]);
        own.shininess = m[3];
        own.specular = m[4];
        own.transparency = m[5];
        own.refractiveIndex = m[6];
        HitInfo hit{HitType::NONE, 0.0, 0, own, normal, Vec3(p[0], p[1], p[2])};
        push(scene.directLightning(hit, view, normal, bias));
        hit.material.color = Vec3(1.0, 1.0, 1.0);
        hit.material.specular = 0.0;
        push(scene.directLightning(hit, view, normal, bias));
        if (own.specular > 0.0) {
            hit.material.color = Vec3(0.0, 0.0, 0.0);
            hit.material.specular = 1.0;
            push(scene.directLightning(hit, view, normal, bias));
        } else {
            push(Vec3(0.0, 0.0, 0.0));
        }
    }
    write_bytes(argv[7], out.data(), out.size() * sizeof(double));
    return 0;
}

int mode_ppm(int argc, char** argv) {
    if (argc < 6) return 1;
    size_t w = std::strtoull(argv[3], nullptr, 10), h = std::strtoull(argv[4], nullptr, 10);
    std::vector<uint8_t> raw(w * h * 3);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(raw.data(), 1, raw.size(), f) != raw.size()) return 2;
    std::fclose(f);
    std::vector<Color> px(w * h);
    for (size_t i = 0; i < px.size(); ++i) px[i] = Color(raw[3 * i], raw[3 * i + 1], raw[3 * i + 2]);
    writePPM(argv[5], px, w, h);
    return 0;
}

// The reference application's OBJ import (RaytracingEngine.cpp:15-65, tinyobjloader): the
// triangles of the loaded model, 9 doubles each (v0, v1, v2; identity transform).
int mode_obj(int argc, char** argv) {
    if (argc < 4) return 1;
    const Model m = LoadObject(argv[2], Transform(), Material());
    std::vector<double> out;
    for (const Triangle& t : m.GetTrianglesFromModel(Material())) {
        for (const Vec3& v : {t.tv0(), t.tv1(), t.tv2()}) {
            out.push_back(v.x);
            out.push_back(v.y);
            out.push_back(v.z);
        }
    }
    write_bytes(argv[3], out.data(), out.size() * sizeof(double));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: ref_harness render|tonemap|curves|kat|closest|trace|anybefore|transmit|"
                             "direct|ppm|obj ...\n");
        return 1;
    }
    std::string m = argv[1];
    if (m == "version") {
#ifdef HARNESS_SHA
        std::printf("%s\n", HARNESS_SHA);
#endif
        return 0;
    }
    int rc = 1;
    if (m == "render") rc = mode_render(argc, argv);
    else if (m == "tonemap") rc = mode_tonemap(argc, argv);
    else if (m == "curves") rc = mode_curves(argc, argv);
    else if (m == "kat") rc = mode_kat(argc, argv);
    else if (m == "closest") rc = mode_closest(argc, argv);
    else if (m == "trace") rc = mode_trace(argc, argv);
    else if (m == "anybefore") rc = mode_anybefore(argc, argv);
    else if (m == "transmit") rc = mode_transmit(argc, argv);
    else if (m == "direct") rc = mode_direct(argc, argv);
    else if (m == "ppm") rc = mode_ppm(argc, argv);
    else if (m == "obj") rc = mode_obj(argc, argv);
    if (rc == 1) std::fprintf(stderr, "bad arguments for mode %s\n", m.c_str());
    return rc;
}
