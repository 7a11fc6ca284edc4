// rtamd/scene.cpp — Scene methods over the C-ABI (see scene.hpp for the mapping).
#include "rtamd/scene.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>

namespace rtamd {

void check(rt_status st, const char* what) {
    if (st != RT_OK) throw std::runtime_error(std::string(what) + ": " + rt_last_error());
}

namespace {
struct ThreadContexts {
    std::map<int, rt_context*> by_device;
    ~ThreadContexts() {
        for (auto& kv : by_device) rt_context_destroy(kv.second);
    }
};
thread_local ThreadContexts t_contexts;
thread_local int t_device = 0;  // the device this thread's last Scene render ran on

void put3(double* d, const Vec3& v) {
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
}
rt_material material_desc(const Material& m) {
    rt_material o;
    put3(o.color, m.color);
    o.shininess = m.shininess;
    o.specular = m.specular;
    o.transparency = m.transparency;
    o.refractive_index = m.refractiveIndex;
    return o;
}
}  // namespace

int current_device() { return t_device; }

rt_context* thread_context(int device) {
    auto it = t_contexts.by_device.find(device);
    if (it != t_contexts.by_device.end()) return it->second;
    rt_context* ctx = nullptr;
    check(rt_context_create(device, &ctx), "rt_context_create");
    t_contexts.by_device[device] = ctx;
    return ctx;
}

// A Scene's upload on one device; remembers which Scene version it holds.
struct SceneDevice {
    int device = -1;
    rt_context* ctx = nullptr;
    rt_scene* scene = nullptr;
    uint64_t version = 0;
    std::vector<long> triangle_owner;  // flat triangle -> -1 (standalone) or model index
    std::vector<size_t> triangle_local;  // flat triangle -> index within its owner list
    ~SceneDevice() {
        if (scene) rt_scene_destroy(scene);
    }
};

}  // namespace rtamd

Scene::Scene(const Camera& camera_) : camera(camera_) {}

rt_camera Scene::cameraDesc() const {
    rt_camera c;
    std::memset(&c, 0, sizeof c);
    c.position[0] = camera.position.x;
    c.position[1] = camera.position.y;
    c.position[2] = camera.position.z;
    c.focal = camera.focal;
    c.width = static_cast<uint32_t>(camera.width);
    c.height = static_cast<uint32_t>(camera.height);
    c.aa_samples = camera.antiAliasingAmount;
    c.near_plane = camera.nearPlaneDistance;
    c.far_plane = camera.farPlaneDistance;
    return c;
}

rt_render_opts Scene::optsDesc(int tonemap) const {
    rt_render_opts o;
    rt_render_opts_default(&o);
    o.max_recursion = maxRecursion;
    o.tonemap = tonemap;
    o.seed = camera.jitterSeed;
    return o;
}

rt_scene* Scene::upload() const {
    rtamd::t_device = device_;
    if (dev_ && dev_->version == version_ && dev_->device == device_) return dev_->scene;
    dev_ = uploadTo(device_);
    return dev_->scene;
}

std::shared_ptr<rtamd::SceneDevice> Scene::uploadTo(int device) const {
    using namespace rtamd;
    auto sd = std::make_shared<SceneDevice>();
    sd->device = device;
    sd->ctx = thread_context(device);

    std::vector<rt_sphere> sp(spheres.size());
    for (size_t i = 0; i < spheres.size(); ++i) {
        put3(sp[i].center, spheres[i].getTransform().position);
        sp[i].radius = spheres[i].getRadius();
        sp[i].material = material_desc(spheres[i].getMaterial());
    }
    std::vector<rt_plane> pl(planes.size());
    for (size_t i = 0; i < planes.size(); ++i) {
        put3(pl[i].point, planes[i].GetTransform().position);
        put3(pl[i].normal, planes[i].GetNormal());
        pl[i].material = material_desc(planes[i].GetMaterial());
    }
    // standalone triangles first, then each model's triangles (IntersectClosest order)
    std::vector<rt_triangle> tr;
    auto push_tri = [&](const Triangle& t, long owner, size_t local) {
        rt_triangle r;
        put3(r.v0, t.vertex(0));
        put3(r.v1, t.vertex(1));
        put3(r.v2, t.vertex(2));
        put3(r.translation, t.transformRef().position);
        r.material = material_desc(t.GetMaterial());
        tr.push_back(r);
        sd->triangle_owner.push_back(owner);
        sd->triangle_local.push_back(local);
    };
    for (size_t i = 0; i < triangles.size(); ++i) push_tri(triangles[i], -1, i);
    for (size_t m = 0; m < models.size(); ++m) {
        const auto tris = models[m].GetTrianglesFromModel(models[m].GetMaterial());
        for (size_t k = 0; k < tris.size(); ++k) push_tri(tris[k], static_cast<long>(m), k);
    }
    std::vector<rt_light> lt(lights.size());
    for (size_t i = 0; i < lights.size(); ++i) {
        put3(lt[i].position, lights[i].position);
        put3(lt[i].color, lights[i].color);
        lt[i].intensity = lights[i].intensity;
    }
    rt_scene_desc d;
    d.spheres = sp.data();
    d.n_spheres = static_cast<int32_t>(sp.size());
    d.planes = pl.data();
    d.n_planes = static_cast<int32_t>(pl.size());
    d.triangles = tr.data();
    d.n_triangles = static_cast<int32_t>(tr.size());
    d.lights = lt.data();
    d.n_lights = static_cast<int32_t>(lt.size());
    check(rt_scene_create(sd->ctx, &d, &sd->scene), "rt_scene_create");
    if (areaLight_) check(rt_scene_set_area_light(sd->scene, &*areaLight_), "rt_scene_set_area_light");
    sd->version = version_;
    return sd;
}

bool Scene::renderMulti(const rt_render_opts& o, double* h64, float* h32, uint8_t* h8) const {
    if (devices_.size() < 2) return false;
    if (multi_.size() != devices_.size()) multi_.assign(devices_.size(), nullptr);
    std::vector<rt_context*> ctxs;
    std::vector<rt_scene*> scs;
    for (size_t i = 0; i < devices_.size(); ++i) {
        if (!multi_[i] || multi_[i]->version != version_ || multi_[i]->device != devices_[i])
            multi_[i] = uploadTo(devices_[i]);
        ctxs.push_back(multi_[i]->ctx);
        scs.push_back(multi_[i]->scene);
    }
    const rt_camera cam = cameraDesc();
    rtamd::check(rt_render_multi(ctxs.data(), scs.data(), static_cast<int>(ctxs.size()), &cam,
                                 &o, h64, h32, h8, countRays_ ? &lastStats_ : nullptr),
                 "rt_render_multi");
    return true;
}

std::vector<Vec3> Scene::RenderImage() const {
    const rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    std::vector<Vec3> img(camera.width * camera.height, Vec3(0, 0, 0));
    if (renderMulti(o, reinterpret_cast<double*>(img.data()), nullptr, nullptr)) return img;
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    // Vec3 is three packed doubles: the device writes the reference's vector<Vec3> layout.
    rtamd::check(rt_render(dev_->ctx, sc, &cam, &o, reinterpret_cast<double*>(img.data()), nullptr,
                           nullptr, countRays_ ? &lastStats_ : nullptr),
                 "rt_render");
    return img;
}

std::vector<Color> Scene::RenderImageTonemapped(int op) const {
    const rt_render_opts o = optsDesc(op);
    std::vector<Color> img(camera.width * camera.height);
    if (renderMulti(o, nullptr, nullptr, reinterpret_cast<uint8_t*>(img.data()))) return img;
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    rtamd::check(rt_render(dev_->ctx, sc, &cam, &o, nullptr, nullptr,
                           reinterpret_cast<uint8_t*>(img.data()), countRays_ ? &lastStats_ : nullptr),
                 "rt_render");
    return img;
}

std::vector<float> Scene::RenderImageF32() const {
    const rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    std::vector<float> img(camera.width * camera.height * 3);
    if (renderMulti(o, nullptr, img.data(), nullptr)) return img;
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    rtamd::check(rt_render(dev_->ctx, sc, &cam, &o, nullptr, img.data(), nullptr, countRays_ ? &lastStats_ : nullptr),
                 "rt_render");
    return img;
}

rtamd::GBuffer Scene::RenderGBuffer(int outputs) const {
    rtamd::GBuffer gb;
    gb.width = camera.width;
    gb.height = camera.height;
    const size_t n = camera.width * camera.height;
    if (outputs & RT_GB_DEPTH) gb.depth.resize(n);
    if (outputs & RT_GB_DEPTH_NORM) gb.depth_norm.resize(n);
    if (outputs & RT_GB_NORMAL) gb.normal.resize(n, Vec3(0, 0, 0));
    if (outputs & RT_GB_PRIM) gb.prim.resize(2 * n);
    if (outputs & RT_GB_ALBEDO) gb.albedo.resize(3 * n);
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    const rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    const rt_gbuffer_out out{gb.depth.data(), gb.depth_norm.data(), gb.normal.data(),
                             gb.prim.data(), gb.albedo.data()};
    rtamd::check(rt_gbuffer(dev_->ctx, sc, &cam, &o, outputs, &out), "rt_gbuffer");
    return gb;
}

Vec3 Scene::GeneratePixelAt(int x, int y) const {
    if (x < 0 || y < 0 || static_cast<size_t>(x) >= camera.width ||
        static_cast<size_t>(y) >= camera.height)
        throw std::out_of_range("GeneratePixelAt: pixel outside the image");
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.row_begin = static_cast<uint32_t>(y);
    o.row_end = static_cast<uint32_t>(y) + 1;
    std::vector<Vec3> row(camera.width, Vec3(0, 0, 0));
    rtamd::check(rt_render(dev_->ctx, sc, &cam, &o, reinterpret_cast<double*>(row.data()),
                           nullptr, nullptr, nullptr),
                 "rt_render");
    return row[static_cast<size_t>(x)];
}

std::optional<Vec3> Scene::GenerateAntiAliasing(size_t x, size_t y, bool isActive,
                                                double bias) const {
    rt_scene* sc = upload();
    const Rayon ray = camera.getRay(x, y, isActive);
    const double r[6] = {ray.origin.x, ray.origin.y, ray.origin.z,
                         ray.direction.x, ray.direction.y, ray.direction.z};
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.bias = bias;
    double rgb[3];
    rtamd::check(rt_trace_rays(dev_->ctx, sc, &o, r, 1, rgb, nullptr), "rt_trace_rays");
    return Vec3(rgb[0], rgb[1], rgb[2]);
}

std::optional<HitInfo> Scene::IntersectClosest(const Rayon& ray) const {
    rt_scene* sc = upload();
    const double r[6] = {ray.origin.x, ray.origin.y, ray.origin.z,
                         ray.direction.x, ray.direction.y, ray.direction.z};
    double h[9];
    rtamd::check(rt_intersect_rays(dev_->ctx, sc, r, 1, h), "rt_intersect_rays");
    const int type = static_cast<int>(h[0]);
    if (type == 0) return std::nullopt;
    const size_t idx = static_cast<size_t>(h[1]);
    const Material none;
    HitInfo hit{HitType::NONE, h[2], idx, none, Vec3(h[3], h[4], h[5]), Vec3(h[6], h[7], h[8])};
    if (type == 1) {
        hit.type = HitType::SPHERE;
        hit.material = spheres[idx].getMaterial();
    } else if (type == 2) {
        hit.type = HitType::PLANE;
        hit.material = planes[idx].GetMaterial();
    } else {
        hit.type = HitType::TRIANGLE;
        const long owner = dev_->triangle_owner[idx];
        if (owner < 0) {
            hit.index = dev_->triangle_local[idx];
            hit.material = triangles[hit.index].GetMaterial();
        } else {  // the reference reports the model's index for model hits (Scene.h:251-253)
            hit.index = static_cast<size_t>(owner);
            hit.material = models[hit.index].GetMaterial();
        }
    }
    return hit;
}

bool Scene::IntersectAnyBefore(const Rayon& ray, double maxDist) const {
    auto within = [&](const std::optional<double>& d) { return d && *d > 0.0 && *d < maxDist; };
    for (const auto& s : spheres)
        if (within(s.Intersect(ray))) return true;
    for (const auto& p : planes)
        if (within(p.Intersect(ray))) return true;
    for (const auto& t : triangles)
        if (within(t.Intersect(ray))) return true;
    for (const auto& m : models)
        if (within(m.Intersect(ray))) return true;
    return false;
}

std::vector<uint8_t> Scene::IntersectAnyBefore(const std::vector<Rayon>& rays,
                                               const std::vector<double>& maxDist) const {
    if (maxDist.size() != rays.size())
        throw std::invalid_argument("IntersectAnyBefore: one maxDist per ray");
    std::vector<uint8_t> out(rays.size());
    if (rays.empty()) return out;
    rt_scene* sc = upload();
    // Rayon is two Vec3 of three packed doubles: the {ox,oy,oz,dx,dy,dz} records of the C-ABI
    static_assert(sizeof(Rayon) == 6 * sizeof(double), "Rayon is not six packed doubles");
    rtamd::check(rt_occluded_rays(dev_->ctx, sc, nullptr,
                                  reinterpret_cast<const double*>(rays.data()), maxDist.data(),
                                  rays.size(), out.data()),
                 "rt_occluded_rays");
    return out;
}

std::vector<uint8_t> Scene::IntersectAnyBefore(const std::vector<Rayon>& rays,
                                               double maxDist) const {
    return IntersectAnyBefore(rays, std::vector<double>(rays.size(), maxDist));
}

double Scene::ComputeTransmittance(const Rayon& ray, double maxDist, double bias) const {
    // the closest hit of IntersectClosest's visiting order (spheres, planes, triangles, models;
    // a later shape wins only when strictly closer), kept as its distance and transparency
    auto closest = [&](const Rayon& r, double& t, double& transparency) {
        bool found = false;
        auto offer = [&](const std::optional<double>& d, const Material& m) {
            if (d && (!found || *d < t)) {
                found = true;
                t = *d;
                transparency = m.transparency;
            }
        };
        for (const auto& s : spheres) offer(s.Intersect(r), s.getMaterial());
        for (const auto& p : planes) offer(p.Intersect(r), p.GetMaterial());
        for (const auto& tr : triangles) offer(tr.Intersect(r), tr.GetMaterial());
        for (const auto& m : models) offer(m.Intersect(r), m.GetMaterial());
        return found;
    };
    double T = 1.0, traveled = 0.0;
    Rayon r = ray;
    for (int step = 0; step < 64 && T > 1e-4 && traveled < maxDist; ++step) {
        double t = 0.0, transparency = 0.0;
        if (!closest(r, t, transparency)) break;
        if (t <= 0.0) {  // a plane under the origin: step off it, nothing is counted
            r.origin = r.origin + r.direction * bias;
            traveled += bias;
            continue;
        }
        if (!(t <= bias)) {  // a hit within the bias is stepped over uncounted too
            if (traveled + t >= maxDist) break;
            T *= std::clamp(transparency, 0.0, 1.0);
        }
        r.origin = r.pointAtDistance(t) + r.direction * bias;
        traveled += t + bias;
    }
    return std::clamp(T, 0.0, 1.0);
}

std::vector<double> Scene::ComputeTransmittance(const std::vector<Rayon>& rays,
                                                const std::vector<double>& maxDist,
                                                double bias) const {
    if (maxDist.size() != rays.size())
        throw std::invalid_argument("ComputeTransmittance: one maxDist per ray");
    std::vector<double> out(rays.size());
    if (rays.empty()) return out;
    rt_scene* sc = upload();
    static_assert(sizeof(Rayon) == 6 * sizeof(double), "Rayon is not six packed doubles");
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.bias = bias;
    rtamd::check(rt_transmittance_rays(dev_->ctx, sc, &o,
                                       reinterpret_cast<const double*>(rays.data()),
                                       maxDist.data(), rays.size(), out.data()),
                 "rt_transmittance_rays");
    return out;
}

std::vector<double> Scene::ComputeTransmittance(const std::vector<Rayon>& rays, double maxDist,
                                                double bias) const {
    return ComputeTransmittance(rays, std::vector<double>(rays.size(), maxDist), bias);
}

namespace {
// The C-ABI record of `keys` for n elements: no pixel keys (element i draws with pixel = i), or
// one per element.
rt_area_keys areaKeysDesc(const rtamd::AreaKeys& keys, size_t n, const char* who) {
    if (!keys.pixel.empty() && keys.pixel.size() != n)
        throw std::invalid_argument(std::string(who) + ": no pixel keys, or one per element");
    return rt_area_keys{keys.pixel.empty() ? nullptr : keys.pixel.data(), keys.sample, keys.depth};
}
}  // namespace

std::vector<double> Scene::LightTransmittance(const std::vector<Vec3>& points,
                                              const std::vector<Vec3>& normals,
                                              double bias) const {
    return lightTransmittance(points, normals, bias, nullptr);
}

std::vector<double> Scene::LightTransmittance(const std::vector<Vec3>& points,
                                              const std::vector<Vec3>& normals,
                                              const rtamd::AreaKeys& keys, double bias) const {
    return lightTransmittance(points, normals, bias, &keys);
}

std::vector<double> Scene::lightTransmittance(const std::vector<Vec3>& points,
                                              const std::vector<Vec3>& normals, double bias,
                                              const rtamd::AreaKeys* keys) const {
    if (normals.size() != points.size())
        throw std::invalid_argument("LightTransmittance: one normal per point");
    const size_t cols =
        lights.size() + (keys && areaLight_ ? static_cast<size_t>(areaLight_->samples) : 0);
    std::vector<double> out(points.size() * cols);
    if (out.empty()) return out;
    rt_scene* sc = upload();
    std::vector<double> pn(6 * points.size());
    for (size_t i = 0; i < points.size(); ++i) {
        const double rec[6] = {points[i].x, points[i].y, points[i].z,
                               normals[i].x, normals[i].y, normals[i].z};
        std::copy(rec, rec + 6, pn.begin() + 6 * i);
    }
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.bias = bias;
    if (keys) {
        const rt_area_keys k = areaKeysDesc(*keys, points.size(), "LightTransmittance");
        rtamd::check(rt_light_transmittance_keyed(dev_->ctx, sc, &o, pn.data(), points.size(),
                                                  out.data(), &k),
                     "rt_light_transmittance_keyed");
    } else {
        rtamd::check(rt_light_transmittance(dev_->ctx, sc, &o, pn.data(), points.size(),
                                            out.data()),
                     "rt_light_transmittance");
    }
    return out;
}

std::optional<HitInfo> Scene::IntersectClosestHost(const Rayon& ray) const {
    std::optional<HitInfo> best;
    auto offer = [&](const std::optional<HitInfo>& h) {
        if (h && (!best || h->isCloserThan(*best))) best = h;
    };
    for (size_t i = 0; i < spheres.size(); ++i) offer(spheres[i].GetHitInfoAt(ray, i));
    for (size_t i = 0; i < planes.size(); ++i) offer(planes[i].GetHitInfoAt(ray, i));
    for (size_t i = 0; i < triangles.size(); ++i) offer(triangles[i].GetHitInfoAt(ray, i));
    for (size_t i = 0; i < models.size(); ++i) offer(models[i].GetHitInfoAt(ray, i));
    return best;
}

Vec3 Scene::DirectLightning(const HitInfo& hit, const Vec3& viewDir, const Vec3& normalIn,
                            double bias) const {
    const Material& material = hit.material;
    const Vec3 normal = normalIn.normalize();
    Vec3 diffuseAccumulation(0, 0, 0), specularAccumulation(0, 0, 0);
    for (const Light& light : lights) {
        const Vec3 vecToLight = light.position - hit.hitPoint;
        const double distanceToLight = vecToLight.length();
        if (distanceToLight <= 0.0) continue;
        const Vec3 lightToHit = vecToLight / distanceToLight;
        const double normalDotLightHit = std::max(0.0, normal.dot(lightToHit));
        if (normalDotLightHit <= 0.0) continue;
        if (distanceToLight <= bias) continue;
        const Rayon shadowRay{hit.hitPoint + normal * bias, lightToHit};
        const double transmittance = ComputeTransmittance(shadowRay, distanceToLight - bias, bias);
        if (transmittance <= bias) continue;
        const Vec3 emitted = light.color * light.intensity;
        const Vec3 contribution =
            emitted * (1.0 / (distanceToLight * distanceToLight)) * normalDotLightHit;
        diffuseAccumulation += contribution * transmittance;
        if (material.transparency <= 0.0 && material.specular > 0.0) {
            const Vec3 halfVector = (lightToHit + viewDir).normalize();
            const double NdotH = std::max(0.0, normal.dot(halfVector));
            if (NdotH > 0.0) {
                const double specFactor = std::pow(NdotH, material.shininess);
                specularAccumulation +=
                    (emitted * (1.0 / (distanceToLight * distanceToLight))) * specFactor * transmittance;
            }
        }
    }
    return material.color * diffuseAccumulation + specularAccumulation * material.specular;
}

static std::vector<Vec3> unpackVec3(const std::vector<double>& v) {
    std::vector<Vec3> out;
    out.reserve(v.size() / 3);
    for (size_t i = 0; i + 2 < v.size(); i += 3) out.emplace_back(v[i], v[i + 1], v[i + 2]);
    return out;
}

std::vector<Vec3> Scene::DirectLightning(const std::vector<HitInfo>& hits,
                                         const std::vector<Vec3>& viewDirs,
                                         const std::vector<Vec3>& normals, double bias) const {
    return directLightning(hits, viewDirs, normals, bias, nullptr);
}

std::vector<Vec3> Scene::DirectLightning(const std::vector<HitInfo>& hits,
                                         const std::vector<Vec3>& viewDirs,
                                         const std::vector<Vec3>& normals,
                                         const rtamd::AreaKeys& keys, double bias) const {
    return directLightning(hits, viewDirs, normals, bias, &keys);
}

std::vector<Vec3> Scene::directLightning(const std::vector<HitInfo>& hits,
                                         const std::vector<Vec3>& viewDirs,
                                         const std::vector<Vec3>& normals, double bias,
                                         const rtamd::AreaKeys* keys) const {
    if (viewDirs.size() != hits.size() || normals.size() != hits.size())
        throw std::invalid_argument("DirectLightning: one viewDir and one normal per hit");
    const size_t n = hits.size();
    if (n == 0) return {};
    rt_scene* sc = upload();
    std::vector<double> pts(9 * n);
    std::vector<rt_material> mats(n);
    for (size_t i = 0; i < n; ++i) {
        const Vec3 &p = hits[i].hitPoint, &nr = normals[i], &v = viewDirs[i];
        const double rec[9] = {p.x, p.y, p.z, nr.x, nr.y, nr.z, v.x, v.y, v.z};
        std::copy(rec, rec + 9, pts.begin() + 9 * i);
        const Material& m = hits[i].material;
        mats[i] = rt_material{{m.color.x, m.color.y, m.color.z}, m.shininess, m.specular,
                              m.transparency, m.refractiveIndex};
    }
    std::vector<double> rgb(3 * n);
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.bias = bias;
    const rt_direct_light_out out{rgb.data(), nullptr, nullptr};
    if (keys) {
        const rt_area_keys k = areaKeysDesc(*keys, n, "DirectLightning");
        rtamd::check(rt_direct_light_keyed(dev_->ctx, sc, &o, pts.data(), mats.data(), n, n,
                                           RT_DL_RADIANCE, &out, &k),
                     "rt_direct_light_keyed");
    } else {
        rtamd::check(rt_direct_light(dev_->ctx, sc, &o, pts.data(), mats.data(), n, n,
                                     RT_DL_RADIANCE, &out),
                     "rt_direct_light");
    }
    return unpackVec3(rgb);
}

std::vector<Vec3> Scene::DirectLightning(const std::vector<Rayon>& rays, double bias) const {
    return directLightningRays(rays, bias, nullptr);
}

std::vector<Vec3> Scene::DirectLightning(const std::vector<Rayon>& rays,
                                         const rtamd::AreaKeys& keys, double bias) const {
    return directLightningRays(rays, bias, &keys);
}

std::vector<Vec3> Scene::directLightningRays(const std::vector<Rayon>& rays, double bias,
                                             const rtamd::AreaKeys* keys) const {
    if (rays.empty()) return {};
    rt_scene* sc = upload();
    static_assert(sizeof(Rayon) == 6 * sizeof(double), "Rayon is not six packed doubles");
    std::vector<double> rgb(3 * rays.size());
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.bias = bias;
    const rt_direct_light_out out{rgb.data(), nullptr, nullptr};
    const double* r = reinterpret_cast<const double*>(rays.data());
    if (keys) {
        const rt_area_keys k = areaKeysDesc(*keys, rays.size(), "DirectLightning");
        rtamd::check(rt_direct_light_rays_keyed(dev_->ctx, sc, &o, r, rays.size(), RT_DL_RADIANCE,
                                                &out, &k),
                     "rt_direct_light_rays_keyed");
    } else {
        rtamd::check(rt_direct_light_rays(dev_->ctx, sc, &o, r, rays.size(), RT_DL_RADIANCE, &out),
                     "rt_direct_light_rays");
    }
    return unpackVec3(rgb);
}

rtamd::Scatter Scene::ScatterRays(const std::vector<Rayon>& rays, bool terminal) const {
    return scatterRays(rays, terminal, nullptr);
}

rtamd::Scatter Scene::ScatterRays(const std::vector<Rayon>& rays, const rtamd::AreaKeys& keys,
                                  bool terminal) const {
    return scatterRays(rays, terminal, &keys);
}

rtamd::Scatter Scene::scatterRays(const std::vector<Rayon>& rays, bool terminal,
                                  const rtamd::AreaKeys* keys) const {
    rtamd::Scatter s;
    const size_t n = rays.size();
    if (n == 0) return s;
    rt_scene* sc = upload();
    static_assert(sizeof(Rayon) == 6 * sizeof(double), "Rayon is not six packed doubles");
    s.value.assign(n, Vec3(0, 0, 0));
    s.refraction.assign(n, Rayon(Vec3(0, 0, 0), Vec3(0, 0, 0)));
    s.reflection.assign(n, Rayon(Vec3(0, 0, 0), Vec3(0, 0, 0)));
    s.flags.assign(n, 0);
    std::vector<double> w(2 * n);
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.max_recursion = terminal ? 0 : 1;
    const rt_scatter_out out{s.value.data(), s.refraction.data(), s.reflection.data(), w.data(),
                             s.flags.data()};
    const double* r = reinterpret_cast<const double*>(rays.data());
    if (keys) {
        const rt_area_keys k = areaKeysDesc(*keys, n, "ScatterRays");
        rtamd::check(rt_scatter_rays_keyed(dev_->ctx, sc, &o, r, n, RT_SC_ALL, &out, &k),
                     "rt_scatter_rays_keyed");
    } else {
        rtamd::check(rt_scatter_rays(dev_->ctx, sc, &o, r, n, RT_SC_ALL, &out), "rt_scatter_rays");
    }
    s.refractionWeight.resize(n);
    s.reflectionWeight.resize(n);
    for (size_t i = 0; i < n; ++i) {
        s.refractionWeight[i] = w[2 * i];
        s.reflectionWeight[i] = w[2 * i + 1];
    }
    return s;
}

std::vector<Vec3> Scene::TraceRays(const std::vector<Rayon>& rays, double bias) const {
    if (rays.empty()) return {};
    rt_scene* sc = upload();
    std::vector<Vec3> rgb(rays.size(), Vec3(0, 0, 0));
    rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    o.bias = bias;
    rtamd::check(rt_trace_rays(dev_->ctx, sc, &o, reinterpret_cast<const double*>(rays.data()),
                               rays.size(), reinterpret_cast<double*>(rgb.data()), nullptr),
                 "rt_trace_rays");
    return rgb;
}

std::vector<Rayon> Scene::CameraRays(int sample) const {
    static_assert(sizeof(Rayon) == 6 * sizeof(double), "Rayon is not six packed doubles");
    rtamd::t_device = device_;
    rt_context* ctx = rtamd::thread_context(device_);
    const rt_camera cam = cameraDesc();
    const rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    std::vector<Rayon> rays(camera.width * camera.height, Rayon(Vec3(0, 0, 0), Vec3(0, 0, 0)));
    // with no pixel the entry still checks the camera and the sample
    double none[6];
    rtamd::check(rt_camera_rays(ctx, &cam, &o, sample,
                                rays.empty() ? none : reinterpret_cast<double*>(rays.data())),
                 "rt_camera_rays");
    return rays;
}

void Scene::AccumulateSamples(int begin, int end, std::vector<Vec3>& sum) const {
    static_assert(sizeof(Vec3) == 3 * sizeof(double), "Vec3 is not three packed doubles");
    const size_t n = camera.width * camera.height;
    if (begin == 0) sum.assign(n, Vec3(0, 0, 0));
    else if (sum.size() != n)
        throw std::runtime_error("AccumulateSamples: begin > 0 needs the frame's sum so far");
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    const rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    double none[3];  // with no pixel the entry still checks the camera and the sample range
    rtamd::check(rt_accumulate_samples(dev_->ctx, sc, &cam, &o, begin, end,
                                       sum.empty() ? none : reinterpret_cast<double*>(sum.data())),
                 "rt_accumulate_samples");
}

void Scene::AccumulateAdaptive(int sampleEnd, const rtamd::AdaptiveRule& rule,
                               rtamd::AdaptiveState& state) const {
    const size_t n = camera.width * camera.height;
    const bool fresh = state.sum.empty() && state.moments.empty() && state.counts.empty();
    if (fresh) {
        state.sum.assign(n, Vec3(0, 0, 0));
        state.moments.assign(2 * n, 0.0);
        state.counts.assign(n, 0);
    } else if (state.sum.size() != n || state.moments.size() != 2 * n || state.counts.size() != n) {
        throw std::runtime_error("AccumulateAdaptive: the state is not empty and not the frame's");
    }
    rt_scene* sc = upload();
    const rt_camera cam = cameraDesc();
    const rt_render_opts o = optsDesc(RT_TONEMAP_NONE);
    const rt_adaptive_rule r{rule.tolerance, rule.lumFloor, rule.minSamples, 0};
    double none[3];  // with no pixel the entry still checks the camera, the rule and sampleEnd
    int32_t none_i[1];
    rtamd::check(rt_accumulate_adaptive(dev_->ctx, sc, &cam, &o, &r, fresh ? 1 : 0, sampleEnd,
                                        n ? reinterpret_cast<double*>(state.sum.data()) : none,
                                        n ? state.moments.data() : none,
                                        n ? state.counts.data() : none_i),
                 "rt_accumulate_adaptive");
}

rtamd::Hits Scene::IntersectClosest(const std::vector<Rayon>& rays) const {
    static_assert(sizeof(Rayon) == 6 * sizeof(double), "Rayon is not six packed doubles");
    static_assert(sizeof(rt_material) == 7 * sizeof(double), "rt_material is not seven doubles");
    rtamd::Hits h;
    const size_t n = rays.size();
    if (n == 0) return h;
    rt_scene* sc = upload();
    h.t.resize(n);
    h.prim.resize(2 * n);
    h.normal.assign(n, Vec3(0, 0, 0));
    h.point.assign(n, Vec3(0, 0, 0));
    h.material.resize(n);
    const rt_closest_out out{h.t.data(), h.prim.data(), h.normal.data(), h.point.data(),
                             h.material.data()};
    rtamd::check(rt_closest_rays(dev_->ctx, sc, nullptr, reinterpret_cast<const double*>(rays.data()),
                                 n, RT_CH_ALL, &out),
                 "rt_closest_rays");
    return h;
}

std::optional<HitInfo> Scene::CalculatePixelDepth(size_t x, size_t y, bool aa) const {
    return IntersectClosest(camera.getRay(x, y, aa));
}
