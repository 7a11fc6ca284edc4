// examples/direct_light_scenefile.cpp — direct-lighting queries on a scene file
// (raytracingengine_amd/scene.py format) through the drop-in C++ API, dumped raw for the parity
// tests (tests/test_oracle_direct_light.py, tests/test_gpu_direct_light.py):
//   rays.f64   n rays, six doubles each {ox, oy, oz, dx, dy, dz}
//   -> batch_rays.f64    Scene::DirectLightning(rays): one launch on the GPU
//   -> batch_points.f64  Scene::DirectLightning(hits, viewDirs, normals) on the host closest hits
//                        of the rays: one launch on the GPU
//   -> single.f64        Scene::DirectLightning(hit, viewDir, normal) per hit: the host utility
// three doubles per ray, directLightning's colour at the ray's first hit; zeros where it misses.
// --host-only writes single.f64 alone and needs no device.
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

static void dump(const std::string& path, const std::vector<Vec3>& v) {
    static_assert(sizeof(Vec3) == 3 * sizeof(double), "Vec3 is not three packed doubles");
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()),
            static_cast<std::streamsize>(v.size() * sizeof(Vec3)));
}

int main(int argc, char** argv) {
    const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
    if (argc - (host_only ? 1 : 0) < 4) {
        std::cerr << "usage: direct_light_scenefile [--host-only] <scene.txt> <rays.f64> <outdir>\n";
        return 2;
    }
    char** a = argv + (host_only ? 1 : 0);
    const std::string out = a[3];
    try {
        const rtamd::LoadedScene L = rtamd::load_scene_file(a[1]);
        const Scene scene = L.build();
        const std::vector<double> r = load(a[2]);
        if (r.size() % 6) throw std::runtime_error("six doubles per ray expected");
        std::vector<Rayon> rays;
        rays.reserve(r.size() / 6);
        for (size_t i = 0; i + 5 < r.size(); i += 6)
            rays.emplace_back(Vec3(r[i], r[i + 1], r[i + 2]), Vec3(r[i + 3], r[i + 4], r[i + 5]));
        // TraceRay's hit, normal and view (Scene.h:136-147) on the host
        std::vector<size_t> at;  // the rays that hit
        std::vector<HitInfo> hits;
        std::vector<Vec3> views, normals;
        for (size_t i = 0; i < rays.size(); ++i) {
            const auto hit = scene.IntersectClosestHost(rays[i]);
            if (!hit) continue;
            const Vec3 incoming = rays[i].direction.normalize();
            const bool frontFace = hit->normal.dot(incoming) < 0.0;
            at.push_back(i);
            hits.push_back(*hit);
            normals.push_back(frontFace ? hit->normal : -hit->normal);
            views.push_back(-incoming);
        }
        std::vector<Vec3> single(rays.size(), Vec3(0, 0, 0));
        for (size_t k = 0; k < at.size(); ++k)
            single[at[k]] = scene.DirectLightning(hits[k], views[k], normals[k]);
        dump(out + "/single.f64", single);
        if (host_only) return 0;
        dump(out + "/batch_rays.f64", scene.DirectLightning(rays));
        const std::vector<Vec3> shaded = scene.DirectLightning(hits, views, normals);
        std::vector<Vec3> points(rays.size(), Vec3(0, 0, 0));
        for (size_t k = 0; k < at.size(); ++k) points[at[k]] = shaded[k];
        dump(out + "/batch_points.f64", points);
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
