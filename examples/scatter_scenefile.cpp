// examples/scatter_scenefile.cpp — the scatter query on a scene file
// (raytracingengine_amd/scene.py format) through the drop-in C++ API, printed and dumped raw for
// the parity tests (tests/test_gpu_scatter.py):
//   rays.f64   n rays, six doubles each {ox, oy, oz, dx, dy, dz}
//   -> value.f64, refraction.f64, reflection.f64 (3, 6, 6 doubles per ray), weights.f64
//      ({refractionWeight, reflectionWeight} per ray) and flags.u8: Scene::ScatterRays(rays),
//      one TraceRay level per ray before its children are traced
// --depth D also composes TraceRay level by level from ScatterRays down to maxRecursion = D,
//   -> composed.f64, and traced.f64: Scene::TraceRays(rays) with SetMaxRecursion(D)
// and prints the two colours next to each other.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "Scene.h"
#include "rtamd/scenefile.hpp"

static std::vector<double> load(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() % sizeof(double)) throw std::runtime_error(path + ": not a file of doubles");
    std::vector<double> v(raw.size() / sizeof(double));
    std::copy(raw.begin(), raw.end(), reinterpret_cast<char*>(v.data()));
    return v;
}

template <class T>
static void dump(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

// TraceRay(ray, level) with maxRecursion = depth, from ScatterRays alone: value, then the
// refraction child times its weight, then the reflection child times its (Scene.h:172, 182, 193).
static std::vector<Vec3> compose(const Scene& scene, const std::vector<Rayon>& rays, int depth,
                                 int level = 0) {
    if (level >= depth) return scene.ScatterRays(rays, true).value;
    const rtamd::Scatter s = scene.ScatterRays(rays);
    std::vector<Vec3> total = s.value;
    for (int child = 0; child < 2; ++child) {
        const uint8_t bit = child == 0 ? 2 : 4;
        const std::vector<Rayon>& all = child == 0 ? s.refraction : s.reflection;
        const std::vector<double>& w = child == 0 ? s.refractionWeight : s.reflectionWeight;
        std::vector<size_t> at;
        std::vector<Rayon> live;
        for (size_t i = 0; i < rays.size(); ++i)
            if (s.flags[i] & bit) {
                at.push_back(i);
                live.push_back(all[i]);
            }
        if (live.empty()) continue;
        const std::vector<Vec3> c = compose(scene, live, depth, level + 1);
        for (size_t k = 0; k < at.size(); ++k) total[at[k]] += c[k] * w[at[k]];
    }
    return total;
}

int main(int argc, char** argv) {
    int depth = -1;
    std::vector<const char*> a;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--depth") == 0 && i + 1 < argc) depth = std::atoi(argv[++i]);
        else a.push_back(argv[i]);
    }
    if (a.size() != 3) {
        std::cerr << "usage: scatter_scenefile [--depth D] <scene.txt> <rays.f64> <outdir>\n";
        return 2;
    }
    const std::string out = a[2];
    try {
        const rtamd::LoadedScene L = rtamd::load_scene_file(a[0]);
        Scene scene = L.build();
        const std::vector<double> r = load(a[1]);
        if (r.size() % 6) throw std::runtime_error("six doubles per ray expected");
        std::vector<Rayon> rays;
        rays.reserve(r.size() / 6);
        for (size_t i = 0; i + 5 < r.size(); i += 6)
            rays.emplace_back(Vec3(r[i], r[i + 1], r[i + 2]), Vec3(r[i + 3], r[i + 4], r[i + 5]));
        static_assert(sizeof(Vec3) == 3 * sizeof(double) && sizeof(Rayon) == 6 * sizeof(double),
                      "Vec3 and Rayon are not packed doubles");
        const rtamd::Scatter s = scene.ScatterRays(rays);
        std::vector<double> w(2 * rays.size());
        for (size_t i = 0; i < rays.size(); ++i) {
            w[2 * i] = s.refractionWeight[i];
            w[2 * i + 1] = s.reflectionWeight[i];
            std::printf("%zu flags %d value %.17g %.17g %.17g fw %.17g rw %.17g\n", i, s.flags[i],
                        s.value[i].x, s.value[i].y, s.value[i].z, w[2 * i], w[2 * i + 1]);
        }
        dump(out + "/value.f64", s.value);
        dump(out + "/refraction.f64", s.refraction);
        dump(out + "/reflection.f64", s.reflection);
        dump(out + "/weights.f64", w);
        dump(out + "/flags.u8", s.flags);
        if (depth >= 0) {
            const std::vector<Vec3> composed = compose(scene, rays, depth);
            scene.SetMaxRecursion(depth);
            const std::vector<Vec3> traced = scene.TraceRays(rays);
            for (size_t i = 0; i < rays.size(); ++i)
                std::printf("%zu composed %.17g %.17g %.17g traced %.17g %.17g %.17g\n", i,
                            composed[i].x, composed[i].y, composed[i].z, traced[i].x, traced[i].y,
                            traced[i].z);
            dump(out + "/composed.f64", composed);
            dump(out + "/traced.f64", traced);
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
