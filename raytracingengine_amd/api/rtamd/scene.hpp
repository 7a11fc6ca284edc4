// rtamd/scene.hpp — the drop-in Scene (/root/reference/RaytracingEngine/Scene.h:14-329).
//
// Same constructor, Add* methods and public query/render methods.  Every method that the
// reference evaluates per pixel runs on the MI355X through the C-ABI (include/rt_capi.h):
//   RenderImage()            → rt_render                (Scene.h:311-328)
//   GeneratePixelAt(x, y)    → rt_render of row y        (Scene.h:283-304)
//   GenerateAntiAliasing(..) → rt_trace_rays             (Scene.h:306-309)
//   IntersectClosest(ray)    → rt_intersect_rays         (Scene.h:218-257)
//   CalculatePixelDepth(..)  → rt_intersect_rays         (Scene.h:278-281)
//   RenderGBuffer()          → rt_gbuffer (extension: CalculatePixelDepth of every pixel)
//   IntersectAnyBefore(rays, maxDist) → rt_occluded_rays  (Scene.h:259-276, for n rays at once)
//   ComputeTransmittance(rays, maxDist, bias) → rt_transmittance_rays (Scene.h:35-77, private
//                              in the reference, for n rays at once)
//   LightTransmittance(points, normals, bias) → rt_light_transmittance (Scene.h:86-104)
//   DirectLightning(hits, viewDirs, normals, bias) → rt_direct_light (Scene.h:79-129, private
//                              in the reference, for n surface points at once)
//   DirectLightning(rays, bias) → rt_direct_light_rays (TraceRay's localLight, Scene.h:136-147, 168)
//   ScatterRays(rays, terminal) → rt_scatter_rays (one TraceRay level, Scene.h:131-198, before
//                              its children are traced)
//   TraceRays(rays, bias)      → rt_trace_rays (TraceRay(ray, 0, bias) for n rays at once)
//   CameraRays(sample)         → rt_camera_rays (Camera::getRay for every pixel, Math.h:99-121)
//   IntersectClosest(rays)     → rt_closest_rays (Scene.h:218-257 for n rays at once)
//   AccumulateSamples(b, e, sum) → rt_accumulate_samples (GeneratePixelAt's sample loop,
//                              Scene.h:289-297, for a range of its samples; rtamd::resolve in
//                              image.hpp divides, Scene.h:298-300)
//   AccumulateAdaptive(end, rule, state) → rt_accumulate_adaptive (that loop, left per pixel by a
//                              stop rule; rtamd::resolve(sum, counts) divides by each count)
// The single-ray IntersectAnyBefore(ray, maxDist) of the reference's signature stays a host
// utility over the shapes' Intersect members: one ray per launch would pay an upload, a launch
// and a download to learn one bit; the batch overloads give the same answers for many rays.
// The single-ray ComputeTransmittance(ray, maxDist, bias) is a host utility for the same reason,
// and so are the single-point DirectLightning(hit, viewDir, normalIn, bias) built on it and
// IntersectClosestHost(ray), the closest hit over the shapes' GetHitInfoAt members.
// Failures throw std::runtime_error(rt_last_error()).
//
// The Add* methods take `const T&` — a compatible superset of the reference's `T&`.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "rtamd/light.hpp"
#include "rtamd/math.hpp"
#include "rt_capi.h"
#include "rtamd/shapes.hpp"

namespace rtamd {
struct SceneDevice;  // uploaded copy of a Scene on one device (scene.cpp)

// The calling thread's context for `device` (created on first use, one per thread+device).
rt_context* thread_context(int device);
// The device of this thread's last single-GPU Scene call (Scene::SetDevice; 0 before any):
// tonemap() / tonemapAll() run there, next to the frame they usually follow.
int current_device();
// Throws std::runtime_error carrying rt_last_error() when st != RT_OK.
void check(rt_status st, const char* what);

// Scene::RenderGBuffer's result: per pixel (row-major, Scene::GetPixelIndex) the HitInfo of
// CalculatePixelDepth(x, y, false).  Outputs that were not requested stay empty.  A miss holds
// prim {0, -1}, depth and depth_norm +inf, normal and albedo 0 (rt_capi.h, G-buffer).
struct GBuffer {
    size_t width = 0, height = 0;
    std::vector<double> depth;       // HitInfo::distance
    std::vector<float> depth_norm;   // (float)HitInfo::normalizedDistance(camera)
    std::vector<Vec3> normal;        // HitInfo::normal (unflipped)
    std::vector<int32_t> prim;       // {type, index} pairs as rt_intersect_rays reports them
    std::vector<float> albedo;       // r g b of HitInfo::material.color
};

// Scene::AccumulateAdaptive's stop rule (rt_adaptive_rule, rt_capi.h): a pixel stops once it has
// minSamples samples and the standard error of its mean luminance is at most tolerance times
// max(mean, lumFloor).
struct AdaptiveRule {
    double tolerance = 0.05;
    double lumFloor = 0.01;
    int minSamples = 4;
};
// ... and its state, one entry per pixel (row-major): the sum of the pixel's samples so far,
// the two luminance moments {m1, m2} the rule reads, and the number of samples taken.
struct AdaptiveState {
    std::vector<Vec3> sum;
    std::vector<double> moments;
    std::vector<int32_t> counts;
};

// Scene::ScatterRays' result: per ray one TraceRay level (Scene.h:131-198) before its children
// are traced (rt_capi.h, rt_scatter_rays).  TraceRay(ray, 0) == value + TraceRay(refraction, 1) *
// refractionWeight + TraceRay(reflection, 1) * reflectionWeight, the children selected by flags.
struct Scatter {
    std::vector<Vec3> value;               // the sky on a miss, else localLight * (1 - transparency)
    std::vector<Rayon> refraction;         // Scene.h:178-180; zeros where absent
    std::vector<Rayon> reflection;         // Scene.h:190-191; zeros where absent
    std::vector<double> refractionWeight;  // transparency * (1 - fresnel); 0 where absent
    std::vector<double> reflectionWeight;  // fresnel, or material.specular; 0 where absent
    std::vector<uint8_t> flags;            // bit 0 hit, bit 1 refraction ray, bit 2 reflection ray
};

// The batch Scene::IntersectClosest's result: per ray the HitInfo members as arrays
// (rt_capi.h, rt_closest_rays).  A miss holds t +inf, prim {0, -1}, zeros elsewhere.
struct Hits {
    std::vector<double> t;              // HitInfo::distance
    std::vector<int32_t> prim;          // {type, index} pairs as rt_intersect_rays reports them
    std::vector<Vec3> normal;           // HitInfo::normal (unflipped)
    std::vector<Vec3> point;            // HitInfo::hitPoint
    std::vector<rt_material> material;  // HitInfo::material, as uploaded
};
// The keys of the area light's draws for a batch of rays or points (rt_area_keys): `pixel` one key
// per element, or empty (element i draws with pixel = i, as TraceRays keys them); `sample` the AA
// sample index and `depth` the recursion depth of the batch.  A frame's draws are keyed by
// pixel = GetPixelIndex(x, y), the sample and the level of the hit.
struct AreaKeys {
    std::vector<uint64_t> pixel;
    uint32_t sample = 0, depth = 0;
};
}  // namespace rtamd

class Scene {
    std::vector<Sphere> spheres;
    std::vector<Plane> planes;
    std::vector<Triangle> triangles;
    std::vector<Model> models;
    std::vector<Light> lights;

    Camera camera;
    int maxRecursion = 10;  // Scene.h:24

    // GPU side (RenderImage is const, so the upload cache is mutable)
    int device_ = 0;
    uint64_t version_ = 1;
    std::optional<rt_area_light> areaLight_;
    mutable std::shared_ptr<rtamd::SceneDevice> dev_;
    mutable rt_stats lastStats_{};
    bool countRays_ = false;

    std::vector<int> devices_;  // > 1 entries: RenderImage over these GPUs (rt_render_multi)
    mutable std::vector<std::shared_ptr<rtamd::SceneDevice>> multi_;

    rt_scene* upload() const;
    std::shared_ptr<rtamd::SceneDevice> uploadTo(int device) const;
    bool renderMulti(const rt_render_opts& o, double* h64, float* h32, uint8_t* h8) const;
    rt_camera cameraDesc() const;
    rt_render_opts optsDesc(int tonemap) const;
    void touch() { ++version_; }
    // the batch queries below with keys (the area light served) or without (nullptr)
    std::vector<double> lightTransmittance(const std::vector<Vec3>& points,
                                           const std::vector<Vec3>& normals, double bias,
                                           const rtamd::AreaKeys* keys) const;
    std::vector<Vec3> directLightning(const std::vector<HitInfo>& hits,
                                      const std::vector<Vec3>& viewDirs,
                                      const std::vector<Vec3>& normals, double bias,
                                      const rtamd::AreaKeys* keys) const;
    std::vector<Vec3> directLightningRays(const std::vector<Rayon>& rays, double bias,
                                          const rtamd::AreaKeys* keys) const;
    rtamd::Scatter scatterRays(const std::vector<Rayon>& rays, bool terminal,
                               const rtamd::AreaKeys* keys) const;

public:
    explicit Scene(const Camera& camera_);

    void AddSphere(const Sphere& sphere) { spheres.emplace_back(sphere); touch(); }
    void AddPlane(const Plane& plane) { planes.emplace_back(plane); touch(); }
    void AddLight(const Light& light) { lights.emplace_back(light); touch(); }
    void AddTriangle(const Triangle& triangle) { triangles.emplace_back(triangle); touch(); }
    void AddModel(const Model& model) { models.emplace_back(model); touch(); }

    size_t GetPixelIndex(size_t x, size_t y) const { return y * camera.width + x; }

    std::optional<HitInfo> IntersectClosest(const Rayon& ray) const;
    bool IntersectAnyBefore(const Rayon& ray, double maxDist) const;
    std::optional<HitInfo> CalculatePixelDepth(size_t x, size_t y, bool aa) const;
    Vec3 GeneratePixelAt(int x, int y) const;
    std::optional<Vec3> GenerateAntiAliasing(size_t x, size_t y, bool isActive, double bias) const;
    std::vector<Vec3> RenderImage() const;

    // ---- extensions (not in the reference) -------------------------------------------
    // Render and tonemap in one launch (fused on the device; `op` is an rt_tonemap_op).
    std::vector<Color> RenderImageTonemapped(int op = RT_TONEMAP_ACES) const;
    // float32 HDR framebuffer (12 B/px) instead of the reference's FP64 Vec3 (24 B/px).
    std::vector<float> RenderImageF32() const;
    // CalculatePixelDepth(x, y, false) for every pixel in one launch (rt_gbuffer): depth,
    // normalised depth, normal, primitive and base colour maps; `outputs` is a set of RT_GB_* bits.
    rtamd::GBuffer RenderGBuffer(int outputs = RT_GB_ALL) const;
    // IntersectAnyBefore(rays[i], maxDist[i]) for every ray in one launch (rt_occluded_rays):
    // 1 or 0 per ray, the answers of the single-ray method above.  maxDist must hold one
    // distance per ray (std::invalid_argument otherwise); the second overload uses one distance
    // for all rays.
    std::vector<uint8_t> IntersectAnyBefore(const std::vector<Rayon>& rays,
                                            const std::vector<double>& maxDist) const;
    std::vector<uint8_t> IntersectAnyBefore(const std::vector<Rayon>& rays, double maxDist) const;
    // computeTransmittance(ray, maxDist, bias) (Scene.h:35-77, private in the reference): the
    // transmittance in [0,1] along the ray up to maxDist — a closest-hit march of at most 64
    // steps over the shapes' Intersect members on the host, the values of the batch overloads.
    double ComputeTransmittance(const Rayon& ray, double maxDist, double bias = 1e-3) const;
    // The same for every ray in one launch (rt_transmittance_rays).  maxDist must hold one
    // distance per ray (std::invalid_argument otherwise); the second overload uses one distance
    // for all rays.
    std::vector<double> ComputeTransmittance(const std::vector<Rayon>& rays,
                                             const std::vector<double>& maxDist,
                                             double bias = 1e-3) const;
    std::vector<double> ComputeTransmittance(const std::vector<Rayon>& rays, double maxDist,
                                             double bias = 1e-3) const;
    // directLightning's shadow rays (Scene.h:86-104) from every point to every point light in one
    // launch (rt_light_transmittance): [i * lights + l], 0.0 where the reference skips the light.
    // normals[i] faces the viewer; one normal per point (std::invalid_argument otherwise).
    std::vector<double> LightTransmittance(const std::vector<Vec3>& points,
                                           const std::vector<Vec3>& normals,
                                           double bias = 1e-3) const;
    // The same with the area light of SetAreaLight served (rt_light_transmittance_keyed):
    // [i * (lights + samples) + c], the area light's samples after the lights, their points drawn
    // under `keys`; the mean of a point's last `samples` values is its soft visibility.  Without
    // an area light: the answer above.
    std::vector<double> LightTransmittance(const std::vector<Vec3>& points,
                                           const std::vector<Vec3>& normals,
                                           const rtamd::AreaKeys& keys, double bias = 1e-3) const;
    // IntersectClosest (Scene.h:218-257) on the host, over the shapes' GetHitInfoAt members in the
    // reference's visiting order (spheres, planes, triangles, models; a later shape wins only
    // when strictly closer): the HitInfo of the device method, without a device.
    std::optional<HitInfo> IntersectClosestHost(const Rayon& ray) const;
    // directLightning(hit, viewDir, normalIn, bias) (Scene.h:79-129, private in the reference) on
    // the host, over the point lights in the reference's operation order, each shadow ray through
    // the host ComputeTransmittance(ray, maxDist, bias): the values of the batch overloads (where
    // std::pow is reached, within an ulp or two of them).  Reads hit.hitPoint and hit.material;
    // normalIn faces the viewer.  The area light of SetAreaLight is not read here; the batch
    // overloads that take rtamd::AreaKeys read it.
    Vec3 DirectLightning(const HitInfo& hit, const Vec3& viewDir, const Vec3& normalIn,
                         double bias = 1e-3) const;
    // The same for every hit in one launch (rt_direct_light): one viewDir and one normal per hit
    // (std::invalid_argument otherwise).
    std::vector<Vec3> DirectLightning(const std::vector<HitInfo>& hits,
                                      const std::vector<Vec3>& viewDirs,
                                      const std::vector<Vec3>& normals, double bias = 1e-3) const;
    // The same with the area light's samples appended after the point lights, drawn under `keys`
    // (rt_direct_light_keyed).
    std::vector<Vec3> DirectLightning(const std::vector<HitInfo>& hits,
                                      const std::vector<Vec3>& viewDirs,
                                      const std::vector<Vec3>& normals, const rtamd::AreaKeys& keys,
                                      double bias = 1e-3) const;
    // directLightning at the first hit of every ray, as TraceRay calls it (Scene.h:136-147, 168),
    // in one launch (rt_direct_light_rays): the hit primitive's material, the normal flipped
    // against the ray, viewDir = -ray.direction.normalize().  (0, 0, 0) where a ray hits nothing.
    std::vector<Vec3> DirectLightning(const std::vector<Rayon>& rays, double bias = 1e-3) const;
    // ... with the area light (rt_direct_light_rays_keyed).
    std::vector<Vec3> DirectLightning(const std::vector<Rayon>& rays, const rtamd::AreaKeys& keys,
                                      double bias = 1e-3) const;
    // One TraceRay level per ray, before its children are traced, in one launch
    // (rt_scatter_rays): what the level adds, the two child rays, their weights and which of them
    // exist.  terminal: every ray is at the recursion limit (Scene.h:132-134): the sky, no
    // intersection, no children — how a caller ends a composition.  The bias is the renderer's
    // (1e-3); maxRecursion is not read, the method never recurses.
    rtamd::Scatter ScatterRays(const std::vector<Rayon>& rays, bool terminal = false) const;
    // The same with the area light in the level's value (rt_scatter_rays_keyed).  RenderImage of
    // an area-light scene composes from it: level k asked with keys.depth = k, keys.sample = the
    // AA sample, and for every ray the pixel key of the camera ray it descends from.
    rtamd::Scatter ScatterRays(const std::vector<Rayon>& rays, const rtamd::AreaKeys& keys,
                               bool terminal = false) const;
    // TraceRay(ray, 0, bias) for every ray in one launch (rt_trace_rays), with maxRecursion.
    std::vector<Vec3> TraceRays(const std::vector<Rayon>& rays, double bias = 1e-3) const;
    // camera.getRay(x, y, sample > 0 && antiAliasingAmount > 1) for every pixel in one launch
    // (rt_camera_rays), row-major (GetPixelIndex): the rays RenderImage traces for AA sample
    // `sample` (0 <= sample < max(1, antiAliasingAmount)), with the device's jitter of that sample.
    std::vector<Rayon> CameraRays(int sample = 0) const;
    // IntersectClosest(rays[i]) for every ray in one launch (rt_closest_rays): the members of the
    // single-ray method's HitInfo as arrays, with the hit primitive's material.  prim holds the
    // C-ABI's {type, index}: a triangle's index counts the standalone triangles first, then each
    // model's.
    rtamd::Hits IntersectClosest(const std::vector<Rayon>& rays) const;
    // Progressive frames (rt_accumulate_samples): for every pixel (row-major, GetPixelIndex),
    // sum += TraceRay(CameraRays(s) of the pixel, 0, bias) for s in [begin, end), GeneratePixelAt's
    // loop (Scene.h:289-297) in its order.  begin == 0 starts the sum (it is resized to the frame
    // and its contents are not read); begin > 0 continues it (it must hold the frame's pixels).
    // 0 <= begin < end <= max(1, antiAliasingAmount).  rtamd::resolve(sum, end) (image.hpp) is the
    // frame after `end` samples; with end = antiAliasingAmount it is RenderImage(), bit for bit.
    void AccumulateSamples(int begin, int end, std::vector<Vec3>& sum) const;
    // AccumulateSamples where every pixel stops by `rule` (rt_accumulate_adaptive): each pixel
    // continues from state.counts up to sampleEnd samples while the rule wants more.  An empty
    // state starts the frame; a state of the frame's size is continued.  1 <= sampleEnd <=
    // max(1, antiAliasingAmount).  rtamd::resolve(state.sum, state.counts) (image.hpp) is the
    // frame; with rule.minSamples >= sampleEnd = antiAliasingAmount it is RenderImage().
    void AccumulateAdaptive(int sampleEnd, const rtamd::AdaptiveRule& rule,
                            rtamd::AdaptiveState& state) const;
    void SetDevice(int device) { device_ = device; dev_.reset(); devices_.clear(); }
    // RenderImage / RenderImageTonemapped / RenderImageF32 over several GPUs of the node from
    // this process: one scene copy per GPU, block-cyclic rows, gathered to the first GPU and
    // copied to the host from there (distinct device ids: one context per device and thread)
    void SetDevices(const std::vector<int>& devices) { devices_ = devices; multi_.clear(); }
    void SetMaxRecursion(int depth) { maxRecursion = depth; }
    // build-defined area light (BASELINE config 5); nullopt removes it
    void SetAreaLight(const std::optional<rt_area_light>& light) { areaLight_ = light; touch(); }
    const Camera& GetCamera() const { return camera; }
    // ray counting (a second, counting launch per render; off by default)
    void SetCountRays(bool on) { countRays_ = on; }
    // ray counts of the last RenderImage* call with counting on (TraceRay reaching
    // IntersectClosest, computeTransmittance calls)
    rt_stats LastStats() const { return lastStats_; }
};
