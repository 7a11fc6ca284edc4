// examples/area_light_scenefile.cpp — the keyed queries on a scene file with an area light
// (raytracingengine_amd/scene.py format, written with area_light=True) through the drop-in C++
// API (tests/test_gpu_area_queries.py):
//   --depth D   composes the frame level by level from Scene::ScatterRays with keys — per AA
//               sample s the camera rays of CameraRays(s), every level k asked with
//               {pixel of the camera ray each ray descends from, s, k} — and prints the maximum
//               difference to RenderImage() with SetMaxRecursion(D), and how many pixels lie
//               beyond 1e-12 * max(1, |RenderImage|)
//   --mask out  writes the soft visibility of the first hits of CameraRays(0) — the mean of the
//               area light's columns of Scene::LightTransmittance with keys — as a binary PGM
//               (0 where a ray hits nothing)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "Scene.h"
#include "rtamd/scenefile.hpp"

// TraceRay(ray, level) with maxRecursion = depth from ScatterRays with keys: value, then the
// refraction child times its weight, then the reflection child times its (Scene.h:172, 182, 193).
static std::vector<Vec3> compose(const Scene& scene, const std::vector<Rayon>& rays,
                                 const std::vector<uint64_t>& pixel, uint32_t sample, int depth,
                                 int level = 0) {
    const rtamd::AreaKeys keys{pixel, sample, static_cast<uint32_t>(level)};
    if (level >= depth) return scene.ScatterRays(rays, keys, true).value;
    const rtamd::Scatter s = scene.ScatterRays(rays, keys);
    std::vector<Vec3> total = s.value;
    for (int child = 0; child < 2; ++child) {
        const uint8_t bit = child == 0 ? 2 : 4;
        const std::vector<Rayon>& all = child == 0 ? s.refraction : s.reflection;
        const std::vector<double>& w = child == 0 ? s.refractionWeight : s.reflectionWeight;
        std::vector<size_t> at;
        std::vector<Rayon> live;
        std::vector<uint64_t> px;
        for (size_t i = 0; i < rays.size(); ++i)
            if (s.flags[i] & bit) {
                at.push_back(i);
                live.push_back(all[i]);
                px.push_back(pixel[i]);
            }
        if (live.empty()) continue;
        const std::vector<Vec3> c = compose(scene, live, px, sample, depth, level + 1);
        for (size_t k = 0; k < at.size(); ++k) total[at[k]] += c[k] * w[at[k]];
    }
    return total;
}

int main(int argc, char** argv) {
    int depth = -1;
    const char* mask = nullptr;
    std::vector<const char*> a;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "--depth") == 0 && i + 1 < argc) depth = std::atoi(argv[++i]);
        else if (std::strcmp(argv[i], "--mask") == 0 && i + 1 < argc) mask = argv[++i];
        else a.push_back(argv[i]);
    }
    if (a.size() != 1 || (depth < 0 && !mask)) {
        std::cerr << "usage: area_light_scenefile [--depth D] [--mask out.pgm] <scene.txt>\n";
        return 2;
    }
    try {
        const rtamd::LoadedScene L = rtamd::load_scene_file(a[0]);
        if (!L.areaLight) throw std::runtime_error("the scene file has no arealight line");
        Scene scene = L.build();
        const size_t w = L.camera.width, h = L.camera.height, n = w * h;
        std::vector<uint64_t> pixel(n);
        for (size_t i = 0; i < n; ++i) pixel[i] = i;  // GetPixelIndex(x, y) of the row-major rays
        if (depth >= 0) {
            scene.SetMaxRecursion(depth);
            const int samples = std::max(1, L.camera.antiAliasingAmount);
            std::vector<Vec3> sum(n, Vec3(0, 0, 0));
            for (int s = 0; s < samples; ++s) {
                const std::vector<Vec3> v =
                    compose(scene, scene.CameraRays(s), pixel, static_cast<uint32_t>(s), depth);
                for (size_t i = 0; i < n; ++i) sum[i] += v[i];
            }
            const std::vector<Vec3> frame = scene.RenderImage();
            double worst = 0.0;
            size_t beyond = 0;
            for (size_t i = 0; i < n; ++i) {
                const Vec3 got = sum[i] / static_cast<double>(samples);
                const double g[3] = {got.x, got.y, got.z}, r[3] = {frame[i].x, frame[i].y, frame[i].z};
                bool out = false;
                for (int c = 0; c < 3; ++c) {
                    const double d = std::fabs(g[c] - r[c]);
                    worst = std::max(worst, d);
                    out = out || !(d <= 1e-12 * std::max(1.0, std::fabs(r[c])));
                }
                beyond += out;
            }
            std::printf("depth %d: max |composed - RenderImage| %.3g, %zu pixels beyond the bar of %zu\n",
                        depth, worst, beyond, n);
        }
        if (mask) {
            const std::vector<Rayon> rays = scene.CameraRays(0);
            const rtamd::Hits hits = scene.IntersectClosest(rays);
            std::vector<Vec3> points, normals;
            rtamd::AreaKeys keys;
            std::vector<size_t> at;
            for (size_t i = 0; i < n; ++i) {
                if (hits.prim[2 * i] == 0) continue;
                const Vec3 inc = rays[i].direction.normalize();
                const Vec3 nrm = hits.normal[i];
                at.push_back(i);
                points.push_back(hits.point[i]);
                normals.push_back(nrm.dot(inc) < 0.0 ? nrm : -nrm);  // facing the viewer
                keys.pixel.push_back(pixel[i]);
            }
            const std::vector<double> T = scene.LightTransmittance(points, normals, keys);
            const size_t al = static_cast<size_t>(L.areaLight->samples);
            const size_t cols = L.lights.size() + al;
            std::vector<unsigned char> img(n, 0);
            for (size_t k = 0; k < at.size(); ++k) {
                double total = 0.0;
                for (size_t s = 0; s < al; ++s) total = total + T[k * cols + L.lights.size() + s];
                img[at[k]] = static_cast<unsigned char>(
                    std::floor(total / static_cast<double>(al) * 255.0 + 0.5));
            }
            std::ofstream f(mask, std::ios::binary);
            f << "P5\n" << w << " " << h << "\n255\n";
            f.write(reinterpret_cast<const char*>(img.data()), static_cast<std::streamsize>(n));
            if (!f) throw std::runtime_error(std::string("cannot write ") + mask);
        }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
