// tbrm_plugin.hpp — C++ host side above the C-ABI (include/tbrm.h), mirroring the plugin's operator surface so that
// code written against the reference reads the same here:
//
//   FDirLightParameters / FClippingPlaneParameters / FRaymarchWorldParameters / FBasicRaymarchRenderingResources
//       Source/Raymarcher/Public/Rendering/RaymarchTypes.h:20-153
//   FWindowingParameters                       Source/VolumeTextureToolkit/Public/VolumeAsset/VolumeInfo.h:31-53
//   URaymarchUtils (static operators)          Source/Raymarcher/Public/Util/RaymarchUtils.h:33-93
//   ARaymarchLight / ARaymarchClipPlane        Source/Raymarcher/Private/Actor/RaymarchLight.cpp:28-31, RaymarchClipPlane.cpp:32-35
//   ARaymarchVolume (Tick / ResetAllLights / UpdateSingleLight / setters)
//       Source/Raymarcher/Private/Actor/RaymarchVolume.cpp:327-465, :630-662, :746-800, :821-949
//
// Header-only, no engine types: FVector/FQuat/FTransform are the ABI PODs. The raymarch itself has no C++ entry point
// in the reference (it is a material on a cube mesh, RaymarchVolume.cpp:37-49); here ARaymarchVolume::RenderLit is the
// offscreen replacement. BASELINE.json spells two of the names URaymarchVolume / FRaymarchResources: both aliases exist.
#pragma once

#include "tbrm.h"
#include "tbrm_labels.h"
#include "tbrm_color_lights.h"
#include "tbrm_volume_region.h"
#include "tbrm_volume_stats.h"
#include "tbrm_hit.h"
#include "tbrm_segment.h"
#include "tbrm_morphology.h"
#include "tbrm_islands.h"
#include "tbrm_margin.h"
#include "tbrm_smooth.h"
#include "tbrm_scissors.h"
#include "tbrm_compete.h"
#include "tbrm_paint.h"
#include "tbrm_surface.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

namespace tbrm_plugin {

using FVector = tbrm_vec3d;
using FQuat = tbrm_quatd;
using FTransform = tbrm_transform;

inline bool operator==(const FVector& a, const FVector& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
inline bool operator!=(const FVector& a, const FVector& b) { return !(a == b); }

// FTransform::Equals with the engine's default tolerances is not reproducible without the engine; exact comparison is
// the conservative choice (any change of the transform requests a recompute, RaymarchVolume.cpp:351).
inline bool TransformEquals(const FTransform& a, const FTransform& b)
{
    return a.rotation.x == b.rotation.x && a.rotation.y == b.rotation.y && a.rotation.z == b.rotation.z &&
           a.rotation.w == b.rotation.w && a.translation == b.translation && a.scale3d == b.scale3d;
}

struct FDirLightParameters { // RaymarchTypes.h:20-41
    FVector LightDirection{0, 0, 0};
    float LightIntensity = 0;
    // Not in the reference (Readme.md:165: "not a RGB light volume to accomodate for colored lights"): the light's colour, white
    // unless set; only a volume with bColoredLights looks at it (include/tbrm_color_lights.h)
    float LightColor[3] = {1.0f, 1.0f, 1.0f};
    FDirLightParameters() = default;
    FDirLightParameters(FVector LightDir, float LightInt) : LightDirection(LightDir), LightIntensity(LightInt) {}
    bool operator==(const FDirLightParameters& rhs) const
    {
        return LightDirection == rhs.LightDirection && LightIntensity == rhs.LightIntensity && LightColor[0] == rhs.LightColor[0] &&
               LightColor[1] == rhs.LightColor[1] && LightColor[2] == rhs.LightColor[2];
    }
    bool operator!=(const FDirLightParameters& rhs) const { return !(*this == rhs); }
    tbrm_dir_light_params abi() const { return tbrm_dir_light_params{LightDirection, LightIntensity, 0}; }
    tbrm_color_dir_light color_abi() const { return tbrm_color_dir_light{abi(), {LightColor[0], LightColor[1], LightColor[2]}, 0}; }
};

struct FClippingPlaneParameters { // RaymarchTypes.h:45-71
    FVector Center{0, 0, 0};
    FVector Direction{0, 0, 0};
    FClippingPlaneParameters() = default;
    FClippingPlaneParameters(FVector ClipCenter, FVector ClipDirection) : Center(ClipCenter), Direction(ClipDirection) {}
    friend bool operator==(const FClippingPlaneParameters& l, const FClippingPlaneParameters& r) { return l.Center == r.Center && l.Direction == r.Direction; }
    friend bool operator!=(const FClippingPlaneParameters& l, const FClippingPlaneParameters& r) { return !(l == r); }
};

struct FRaymarchWorldParameters { // RaymarchTypes.h:136-153
    FTransform VolumeTransform{{0, 0, 0, 1}, {0, 0, 0}, {1, 1, 1}};
    FClippingPlaneParameters ClippingPlaneParameters;
    friend bool operator==(const FRaymarchWorldParameters& l, const FRaymarchWorldParameters& r)
    {
        return TransformEquals(l.VolumeTransform, r.VolumeTransform) && l.ClippingPlaneParameters == r.ClippingPlaneParameters;
    }
    friend bool operator!=(const FRaymarchWorldParameters& l, const FRaymarchWorldParameters& r) { return !(l == r); }
    tbrm_world_params abi() const
    {
        return tbrm_world_params{VolumeTransform, {ClippingPlaneParameters.Center, ClippingPlaneParameters.Direction}};
    }
};

struct FWindowingParameters { // VolumeInfo.h:31-53
    float Center = 0.5f;
    float Width = 1.0f;
    bool LowCutoff = true;
    bool HighCutoff = true;
    tbrm_windowing_params abi() const { return tbrm_windowing_params{Center, Width, LowCutoff ? 1 : 0, HighCutoff ? 1 : 0}; }
};

// UCurveLinearColor restricted to what every shipped TF curve uses: RCIM_Linear keys per channel.
struct FColorCurve {
    std::vector<float> Times[4], Values[4]; // R, G, B, A
    void AddKey(float t, float r, float g, float b, float a)
    {
        const float v[4] = {r, g, b, a};
        for (int c = 0; c < 4; ++c) { Times[c].push_back(t); Values[c].push_back(v[c]); }
    }
};

enum class ERaymarchMaterial { Lit, Intensity, Octree }; // RaymarchVolume.h:24-29

// RaymarchTypes.h:87-129. The GPU objects the reference holds by pointer live behind one opaque handle.
struct FBasicRaymarchRenderingResources {
    bool bIsInitialized = false;
    tbrm_resources* Handle = nullptr; // DataVolumeTextureRef + TFTextureRef + LightVolumeRenderTarget + XYZReadWriteBuffers
    bool LightVolumeHalfResolution = false;
    FWindowingParameters WindowingParameters;
    int SizeX = 0, SizeY = 0, SizeZ = 0; // DataVolumeTextureRef->GetSizeX/Y/Z()
    int DataFormat = TBRM_FMT_G8;        // DataVolumeTextureRef->GetPixelFormat(): what Handle was created with
};
using FRaymarchResources = FBasicRaymarchRenderingResources;

struct URaymarchUtils { // RaymarchUtils.h:33-93; all static, like the Blueprint function library
    static void AddDirLightToSingleVolume(const FBasicRaymarchRenderingResources& Resources, const FDirLightParameters& LightParameters,
                                          const bool Added, const FRaymarchWorldParameters WorldParameters, bool& LightAdded, bool bGPUSync = false)
    {
        const tbrm_dir_light_params l = LightParameters.abi();
        const tbrm_world_params w = WorldParameters.abi();
        int flag = 0;
        tbrm_add_dir_light(Resources.Handle, &l, Added ? 1 : 0, &w, &flag, bGPUSync ? 1 : 0);
        LightAdded = flag != 0;
    }
    // Not in the reference: several AddDirLightToSingleVolume calls as one (tbrm_add_dir_lights: passes of different lights
    // that leave the same cube face share one slice loop). Returns the number of passes that ran paired.
    static int AddDirLightsToSingleVolume(const FBasicRaymarchRenderingResources& Resources, const std::vector<FDirLightParameters>& Lights,
                                          const bool Added, const FRaymarchWorldParameters WorldParameters, bool& LightsAdded)
    {
        std::vector<tbrm_dir_light_params> l;
        for (const FDirLightParameters& p : Lights) l.push_back(p.abi());
        const tbrm_world_params w = WorldParameters.abi();
        std::vector<int32_t> schedule(8 * l.size() + 8);
        int32_t entries = 0;
        LightsAdded = tbrm_add_dir_lights(Resources.Handle, l.data(), (int32_t) l.size(), Added ? 1 : 0, &w, schedule.data(), &entries) == TBRM_OK;
        int paired = 0;
        for (int32_t e = 0; e < entries; ++e) paired += schedule[4 * e + 2] >= 0 ? 2 : 0;
        return paired;
    }
    static void ChangeDirLightInSingleVolume(FBasicRaymarchRenderingResources& Resources, const FDirLightParameters OldLightParameters,
                                             const FDirLightParameters NewLightParameters, const FRaymarchWorldParameters WorldParameters,
                                             bool& LightAdded, bool bGPUSync = false)
    {
        const tbrm_dir_light_params o = OldLightParameters.abi(), n = NewLightParameters.abi();
        const tbrm_world_params w = WorldParameters.abi();
        int flag = 0;
        tbrm_change_dir_light(Resources.Handle, &o, &n, &w, &flag, bGPUSync ? 1 : 0);
        LightAdded = flag != 0;
    }
    // Not in the reference: the two operators with the lights' colours, on a volume with bColoredLights (tbrm_color_lights.h)
    static void AddColorDirLightToSingleVolume(const FBasicRaymarchRenderingResources& Resources, const FDirLightParameters& LightParameters,
                                               const bool Added, const FRaymarchWorldParameters WorldParameters, bool& LightAdded)
    {
        const tbrm_color_dir_light l = LightParameters.color_abi();
        const tbrm_world_params w = WorldParameters.abi();
        int flag = 0;
        tbrm_add_color_dir_light(Resources.Handle, &l, Added ? 1 : 0, &w, &flag);
        LightAdded = flag != 0;
    }
    static void ChangeColorDirLightInSingleVolume(FBasicRaymarchRenderingResources& Resources, const FDirLightParameters OldLightParameters,
                                                  const FDirLightParameters NewLightParameters, const FRaymarchWorldParameters WorldParameters,
                                                  bool& LightAdded)
    {
        const tbrm_color_dir_light o = OldLightParameters.color_abi(), n = NewLightParameters.color_abi();
        const tbrm_world_params w = WorldParameters.abi();
        int flag = 0;
        tbrm_change_color_dir_light(Resources.Handle, &o, &n, &w, &flag);
        LightAdded = flag != 0;
    }
    // RaymarchUtils.cpp:94-102
    static bool GenerateOctree(FBasicRaymarchRenderingResources& Resources)
    {
        return Resources.Handle && tbrm_generate_octree(Resources.Handle) == TBRM_OK;
    }

    static void ClearResourceLightVolumes(FBasicRaymarchRenderingResources Resources, float ClearValue)
    {
        if (!Resources.Handle) return;
        tbrm_clear_light_volume(Resources.Handle, ClearValue);
    }
    // ColorCurveToTexture / MakeDefaultTFTexture produce the 256-sample LUT the handle stores as FFloat16.
    static void ColorCurveToTexture(const FColorCurve& Curve, std::vector<float>& OutTexture)
    {
        OutTexture.assign(256 * 4, 0.0f);
        const float* t[4] = {Curve.Times[0].data(), Curve.Times[1].data(), Curve.Times[2].data(), Curve.Times[3].data()};
        const float* v[4] = {Curve.Values[0].data(), Curve.Values[1].data(), Curve.Values[2].data(), Curve.Values[3].data()};
        const int32_t n[4] = {(int32_t) Curve.Times[0].size(), (int32_t) Curve.Times[1].size(), (int32_t) Curve.Times[2].size(), (int32_t) Curve.Times[3].size()};
        tbrm_color_curve_to_lut(t, v, n, OutTexture.data());
    }
    static void MakeDefaultTFTexture(std::vector<float>& OutTexture)
    {
        OutTexture.assign(256 * 4, 0.0f);
        tbrm_make_default_tf_lut(OutTexture.data());
    }
    // CreateBufferTextures / ReleaseOneAxisReadWriteBufferResources (RaymarchUtils.cpp:176-217): the four read/write
    // buffers per axis belong to the tbrm handle (created with it, released with it: tbrm_resources_create / _destroy), so
    // a host has nothing to create or release; the names are kept so that call sites compile unchanged.
    struct OneAxisReadWriteBufferResources {}; // RaymarchTypes.h:75-81
    static void CreateBufferTextures(int /*SizeX*/, int /*SizeY*/, int /*PixelFormat*/, OneAxisReadWriteBufferResources& /*RWBuffers*/) {}
    static void ReleaseOneAxisReadWriteBufferResources(OneAxisReadWriteBufferResources& /*Buffer*/) {}

    // The Blueprint-pure helpers (RaymarchUtils.cpp:219-252)
    static void GetVolumeTextureDimensions(const FBasicRaymarchRenderingResources* Resources, int32_t Dimensions[3])
    {
        Dimensions[0] = Resources ? Resources->SizeX : 0;
        Dimensions[1] = Resources ? Resources->SizeY : 0;
        Dimensions[2] = Resources ? Resources->SizeZ : 0;
    }
    // FTransform::ToMatrixWithScale / ToMatrixNoScale: row-vector convention, rows 0-2 = scaled rotation axes, row 3 = translation
    static void TransformToMatrix(const FTransform& Transform, double OutMatrix[4][4], bool WithScaling)
    {
        const FQuat& q = Transform.rotation;
        const double sx = WithScaling ? Transform.scale3d.x : 1.0, sy = WithScaling ? Transform.scale3d.y : 1.0, sz = WithScaling ? Transform.scale3d.z : 1.0;
        const double x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
        const double xx = q.x * x2, yy = q.y * y2, zz = q.z * z2, xy = q.x * y2, xz = q.x * z2, yz = q.y * z2, wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
        const double m[4][4] = {{(1.0 - (yy + zz)) * sx, (xy + wz) * sx, (xz - wy) * sx, 0.0},
                                {(xy - wz) * sy, (1.0 - (xx + zz)) * sy, (yz + wx) * sy, 0.0},
                                {(xz + wy) * sz, (yz - wx) * sz, (1.0 - (xx + yy)) * sz, 0.0},
                                {Transform.translation.x, Transform.translation.y, Transform.translation.z, 1.0}};
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) OutMatrix[r][c] = m[r][c];
    }
    static void LocalToTextureCoords(FVector LocalCoords, FVector& TextureCoords) // local cube [-1,1]^3 -> texture [0,1]^3
    {
        TextureCoords = FVector{LocalCoords.x / 2.0 + 0.5, LocalCoords.y / 2.0 + 0.5, LocalCoords.z / 2.0 + 0.5};
    }
    static void TextureToLocalCoords(FVector TextureCoords, FVector& LocalCoords)
    {
        LocalCoords = FVector{(TextureCoords.x - 0.5) * 2.0, (TextureCoords.y - 0.5) * 2.0, (TextureCoords.z - 0.5) * 2.0};
    }
};

struct ARaymarchLight { // direction = actor forward vector (RaymarchLight.cpp:28-31)
    FVector ForwardVector{1, 0, 0};
    float LightIntensity = 1.0f;
    float LightColor[3] = {1.0f, 1.0f, 1.0f}; // (not in the reference) every component in [0, 1]; a change is a Change, like an intensity's
    std::string Name = "RaymarchLight";
    FDirLightParameters GetCurrentParameters() const
    {
        FDirLightParameters p(ForwardVector, LightIntensity);
        for (int c = 0; c < 3; ++c) p.LightColor[c] = LightColor[c];
        return p;
    }
    tbrm_color_dir_light GetCurrentColorParameters() const { return GetCurrentParameters().color_abi(); }
};

struct ARaymarchClipPlane { // (location, -up) (RaymarchClipPlane.cpp:32-35)
    FVector Location{0, 0, 0};
    FVector UpVector{0, 0, 1};
    FClippingPlaneParameters GetCurrentParameters() const { return FClippingPlaneParameters(Location, FVector{-UpVector.x, -UpVector.y, -UpVector.z}); }
};

// What a ray of the lit march meets first (include/tbrm_hit.h; no counterpart in the reference, whose VR controllers point at the
// cube mesh): ARaymarchVolume::PickVolume
struct FVolumeHit {
    bool bHit = false;
    FVector WorldPosition{0, 0, 0};
    double Depth = 0.0;  // along the camera's forward axis, world units (the scene-depth convention); no hit: +inf
    float Value = 0.0f;  // the filtered data value there, in the window's units
    int Label = -1;      // the label volume's voxel there; -1 without a label volume or a hit
    int Sample = -1;     // the sample's index along the ray
    float Uvw[3] = {0, 0, 0}; // the sample's position in the volume's unit cube (tbrm_hit::uvw): what PaintAlongHits strings into a stroke
};

// What a region growing call found (include/tbrm_segment.h): ARaymarchVolume::GrowRegion / GrowRegionAt
struct FGrowResult {
    bool bSeeded = false;          // GrowRegionAt: the ray met the volume (else nothing was grown)
    int Seed[3] = {-1, -1, -1};    // GrowRegionAt: the voxel under the pixel
    uint64_t Voxels = 0;           // the region's size
    uint64_t Relabelled = 0;       // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // inclusive; an empty region: the volume's size and -1
    int Passes = 0;
    double LoUsed = 0.0, HiUsed = 0.0; // the value range applied, in stored units
};

// What a label morphology call found (include/tbrm_morphology.h): ARaymarchVolume::MorphLabel and its four named forms
struct FMorphResult {
    uint64_t SourceVoxels = 0, ResultVoxels = 0; // the label's voxels before and the operator's result, inside the box
    uint64_t Added = 0, Removed = 0;             // voxels that joined / left the label
    uint64_t Relabelled = 0;                     // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of what joined or left, inclusive; nothing: the volume's size and -1
    int Launches = 0;
};

// What a Euclidean margin call found (include/tbrm_margin.h): ARaymarchVolume::MarginLabel and its four named forms
struct FMarginResult {
    uint64_t SourceVoxels = 0, ResultVoxels = 0; // the label's voxels before and the operator's result, inside the box
    uint64_t Added = 0, Removed = 0;             // voxels that joined / left the label
    uint64_t Relabelled = 0;                     // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of what joined or left, inclusive; nothing: the volume's size and -1
    int Reach[3] = {0, 0, 0};                    // voxels per axis the radius reaches
    uint32_t Weights[3] = {0, 0, 0}, Limit = 0;  // the squared distance the radius and the spacing became (tbrm_host_margin_weights)
    int Launches = 0;
};

// What a smoothing call found (include/tbrm_smooth.h): ARaymarchVolume::SmoothLabel and MedianLabel
struct FSmoothResult {
    uint64_t SourceVoxels = 0, ResultVoxels = 0; // the label's voxels before and the filter's result, inside the box
    uint64_t Added = 0, Removed = 0;             // voxels that joined / left the label
    uint64_t Relabelled = 0;                     // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of what joined or left, inclusive; nothing: the volume's size and -1
    int Radius[3] = {0, 0, 0};                   // voxels per axis the radius and the spacing became (tbrm_host_smooth_radii)
    int Reach[3] = {0, 0, 0};                    // Iterations times that
    int Launches = 0;
};

// What a scissors call found (include/tbrm_scissors.h): ARaymarchVolume::ScissorLabel and its kin
struct FScissorsResult {
    uint64_t SourceVoxels = 0, ResultVoxels = 0; // the label's voxels before and afterwards
    uint64_t Added = 0, Removed = 0;             // voxels that joined / left the label
    uint64_t Relabelled = 0;                     // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of what joined or left, inclusive; nothing: the volume's size and -1
    int BricksInside = 0, BricksOutside = 0;     // bricks their corners put wholly under / wholly beside the lasso
    int BricksProjected = 0;                     // bricks projected voxel by voxel
    int Launches = 0;
    uint64_t MaskPixels = 0;                     // pixels of the view inside the lasso
};

// What a grow-from-seeds call found (include/tbrm_compete.h): ARaymarchVolume::GrowFromSeeds
struct FCompeteResult {
    uint64_t SeedVoxels = 0, Claimable = 0, Claimed = 0; // the painted voxels, the voxels they competed for, those a seed reached
    uint64_t Relabelled = 0;                     // label bytes that changed
    uint64_t ClaimedPerLabel[256] = {};
    uint32_t MaxCost = 0;                        // the largest cost of a claimed voxel
    int Passes = 0;
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of the claimed voxels, inclusive; none: the volume's size and -1
    int StepCost[3] = {0, 0, 0};                 // what the call charged per step along each axis
};

// What a brush stroke found (include/tbrm_paint.h): ARaymarchVolume::PaintLabel, EraseLabel and PaintAlongHits
struct FPaintResult {
    uint64_t StampVoxels = 0;                    // voxels of the box within the stroke (and inside the gate)
    uint64_t Added = 0, Removed = 0;             // voxels that joined / left the label
    uint64_t Relabelled = 0;                     // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of what joined or left, inclusive; nothing: the volume's size and -1
    int Points = 0, Segments = 0;                // of the stroke as painted
    int BricksWhole = 0, BricksUntouched = 0, BricksEvaluated = 0;
    int Launches = 0;
    uint32_t Weights[3] = {0, 0, 0}, Limit = 0;  // the squared distance the radius and the spacing became (tbrm_host_paint_brush)
};

// The surface of a label as a mesh (include/tbrm_surface.h): ARaymarchVolume::ExtractLabelSurface / MeasureLabelSurface
struct FLabelSurface {
    std::vector<float> Positions;                // x, y, z per vertex, in the volume's local unit cube (voxel i at i / (N - 1))
    std::vector<float> Normals;                  // x, y, z per vertex: the record's integer normal scaled by the voxel spacing and
                                                 // normalised; (0, 0, 0) where the cell is ambiguous
    std::vector<uint32_t> Triangles;             // three indices each, counter-clockwise seen from outside
    std::vector<tbrm_surface_vertex> Records;    // the exact records the positions come from
    uint64_t SetVoxels = 0, Vertices = 0, Quads = 0;
    uint64_t QuadsAxis[3] = {0, 0, 0};
    int CellMin[3] = {0, 0, 0}, CellMax[3] = {-1, -1, -1}; // of the active cells, inclusive; none: the volume's size and -1
    int BlocksEvaluated = 0, BlocksSkipped = 0, Launches = 0;
};

// The options of a brush stroke; the defaults paint over every label, anywhere, whatever the voxel's value
struct FPaintOptions {
    bool bGate = false;                          // paint only voxels whose stored value lies in Lo .. Hi
    double Lo = 0.0, Hi = 0.0;
    std::vector<int> Writable;                   // the labels a painted voxel may overwrite; empty: every label
    int Origin[3] = {0, 0, 0}, Extent[3] = {0, 0, 0}; // the box; all-zero extent: the whole volume
    int EraseTo = 0;                             // the label of voxels that leave
    bool bMeasureOnly = false;
};

// The options of ARaymarchVolume::GrowFromSeeds; the defaults let every voxel that is no seed be claimed
struct FCompeteOptions {
    double Lo = 0.0, Hi = -1.0;                  // the gate in stored units; Hi < Lo: the format's whole range (float: every finite value)
    int StepCost[3] = {-1, -1, -1};              // per axis, 0 .. 65535; negative: StepCostFromSpacing(SpacingCost)
    int SpacingCost = 16;                        // ... the cost of a step along the axis of the finest spacing
    int ValueShift = 0;
    uint32_t CostLimit = 0;                      // 0: none but the key's, 2^24 - 1
    double FloatLo = 0.0, FloatHi = 1.0;         // R32_FLOAT volumes: the values that become the codes 0 .. 65535
    std::vector<int> Writable;                   // the labels that may be claimed; empty: every label
    int Origin[3] = {0, 0, 0}, Extent[3] = {0, 0, 0}; // the box; all-zero extent: the whole volume
    bool bMeasureOnly = false;
};

// What an island call found (include/tbrm_islands.h): ARaymarchVolume::KeepLargestIslands / RemoveSmallIslands / SplitIslands /
// FillLabelHoles
struct FIslandsResult {
    uint64_t SetVoxels = 0;                      // the voxels the islands were taken of
    uint64_t Islands = 0, Spared = 0;            // islands in the order; islands on a face of the volume left out of it (FillLabelHoles)
    uint64_t Kept = 0, Dropped = 0, KeptVoxels = 0, DroppedVoxels = 0;
    uint64_t Largest = 0;                        // voxels of the largest island
    uint64_t Relabelled = 0;                     // label bytes that changed
    int BoxMin[3] = {0, 0, 0}, BoxMax[3] = {-1, -1, -1}; // of the changed bytes, inclusive; none: the volume's size and -1
};

class ARaymarchVolume {
public:
    // ---- the reflected properties the hot path consumes (RaymarchVolume.h:60-266) ----
    FBasicRaymarchRenderingResources RaymarchResources;
    FRaymarchWorldParameters WorldParameters;
    std::vector<ARaymarchLight*> LightsArray;
    ARaymarchClipPlane* ClippingPlane = nullptr;
    FTransform ComponentTransform{{0, 0, 0, 1}, {0, 0, 0}, {100, 100, 100}}; // the cube mesh component (RaymarchVolume.cpp:47)
    bool bLightVolume32Bit = false;
    bool bFastShader = true; // accepted and ignored: the reference's GPUSync branch is a no-op (RaymarchUtils.cpp:51-59)
    bool bRequestedRecompute = false;
    bool bVisible = true;
    float RaymarchingSteps = 150;
    ERaymarchMaterial SelectRaymarchMaterial = ERaymarchMaterial::Lit;
    int Device = 0;
    int DataAddressMode = TBRM_ADDRESS_WRAP;
    bool bRecordLightsOnReset = false; // see ResetAllLights
    bool bBatchLightsOnReset = false;  // ResetAllLights adds all lights with one batched call (UNORM8 result may differ by one code at fp32 ties)
    // (not in the reference) an RGB light volume lit by the lights' LightColor; read when the resources are initialised
    // (SetVolumeAsset). false: a mono handle, and LightColor is ignored. The batched reset has no colour form: light by light.
    bool bColoredLights = false;
    // (not in the reference) the voxel spacing MarginLabel and SmoothLabel measure their radius in: LoadMHDFileIntoVolume sets it to the file's
    // ElementSpacing, SetVolumeAsset (a new asset, of unknown spacing) resets it; all zero: unit spacing
    double VoxelSpacing[3] = {0, 0, 0};

    struct FStats { int Resets = 0, LightAdds = 0, LightChanges = 0, Frames = 0; } Stats; // what Tick decided (test hook)

    ~ARaymarchVolume() { FreeRaymarchResources(); }

    // SetVolumeAsset (RaymarchVolume.cpp:467-560): UVolumeTexture-shaped buffer in, resources (re)initialised
    bool SetVolumeAsset(const void* Voxels, int SizeX, int SizeY, int SizeZ, int Format)
    {
        InitializeRaymarchResources(SizeX, SizeY, SizeZ, Format);
        for (double& s : VoxelSpacing) s = 0.0;
        if (!RaymarchResources.Handle) return false;
        const size_t bytes = (size_t) SizeX * SizeY * SizeZ * (Format == TBRM_FMT_G8 ? 1 : (Format == TBRM_FMT_G16 ? 2 : 4));
        if (tbrm_upload_volume(RaymarchResources.Handle, Voxels, bytes) != TBRM_OK) return false;
        bRequestedOctreeRebuild = true; // :554
        if (!bHasTF) {
            std::vector<float> lut;
            URaymarchUtils::MakeDefaultTFTexture(lut);
            tbrm_set_tf_lut(RaymarchResources.Handle, lut.data());
            bHasTF = true;
        }
        tbrm_windowing_params w = RaymarchResources.WindowingParameters.abi();
        tbrm_set_windowing(RaymarchResources.Handle, &w);
        RaymarchResources.bIsInitialized = tbrm_resources_is_initialized(RaymarchResources.Handle) != 0;
        // OnConstruction (RaymarchVolume.cpp:161-173): remember the lights' parameters
        LightParametersMap.clear();
        for (ARaymarchLight* Light : LightsArray)
            if (Light && Light->LightIntensity > 0.0f) LightParametersMap[Light] = Light->GetCurrentParameters();
        bRequestedRecompute = true; // :552
        return RaymarchResources.bIsInitialized;
    }

    void SetTFCurve(const FColorCurve& Curve) // :562-577
    {
        if (!RaymarchResources.Handle) return;
        std::vector<float> lut;
        URaymarchUtils::ColorCurveToTexture(Curve, lut);
        tbrm_set_tf_lut(RaymarchResources.Handle, lut.data());
        bHasTF = true;
        bRequestedRecompute = true;
    }

    // A sub-box of the data volume (include/tbrm_volume_region.h; the reference can only set the whole asset again): dense, x
    // fastest, in the asset's format. The light volume was propagated through the old voxels, so the next Tick runs
    // ResetAllLights, as after SetVolumeAsset, and the octree is rebuilt before it is marched again.
    bool UpdateVolumeRegion(const int32_t Origin[3], const int32_t Extent[3], const void* Voxels, size_t NumBytes)
    {
        if (!RaymarchResources.Handle || tbrm_update_volume_region(RaymarchResources.Handle, Origin, Extent, Voxels, NumBytes) != TBRM_OK) return false;
        bRequestedRecompute = true;
        bRequestedOctreeRebuild = true;
        return true;
    }

    // Volume statistics (include/tbrm_volume_stats.h; no counterpart in the reference): computed on the device, where the voxels are.
    // The value histogram of the whole asset in NumBins (1 .. 4096) equal bins, in stored units: over the full code range for the
    // UNORM formats, over [global min, global max] (tbrm_label_statistics) for float data.
    bool ComputeHistogram(int NumBins, std::vector<uint64_t>& Out)
    {
        double Lo = 0.0, Hi = 0.0;
        return HistogramWithRange(NumBins, Out, Lo, Hi);
    }
    // Per label 0 .. 255 (without a label volume: everything under label 0) the voxel count, sum, minimum and maximum.
    bool GetLabelStatistics(std::vector<tbrm_label_stat>& Out)
    {
        Out.assign(256, tbrm_label_stat{});
        return RaymarchResources.Handle && tbrm_label_statistics(RaymarchResources.Handle, nullptr, nullptr, Out.data()) == TBRM_OK;
    }
    // A window from the data instead of the default centre 0.5 / width 1: the span between the two percentiles of the value
    // histogram (256 bins for UNORM8, 1024 for UNORM16 and float; tbrm_host_window_from_histogram has the rule), both cut-offs on.
    // It goes through the setters, so the windowing change reaches the handle and requests the light recompute exactly as a
    // user's slider does. Window units: normalised value for UNORM data, the value itself for float data.
    bool AutoWindow(float LowPercentile = 0.01f, float HighPercentile = 0.99f)
    {
        std::vector<uint64_t> Counts;
        double Lo = 0.0, Hi = 0.0;
        if (!HistogramWithRange(RaymarchResources.DataFormat == TBRM_FMT_G8 ? 256 : 1024, Counts, Lo, Hi)) return false;
        double LoEdge = Lo, HiEdge = Hi;
        if (RaymarchResources.DataFormat != TBRM_FMT_R32_FLOAT) { LoEdge = 0.0; HiEdge = (Hi + 1.0) / Hi; } // bins of codes 0 .. max, in units of code / max
        tbrm_windowing_params w{};
        if (tbrm_host_window_from_histogram(Counts.data(), (int32_t) Counts.size(), LoEdge, HiEdge, LowPercentile, HighPercentile, &w) != TBRM_OK) return false;
        SetWindowCenter(w.center);
        SetWindowWidth(w.width);
        SetLowCutoff(w.low_cutoff != 0);
        SetHighCutoff(w.high_cutoff != 0);
        return true;
    }

    // Label overlay (include/tbrm_labels.h; no counterpart in the reference's actor): thin forwards to the C-ABI. Labels change
    // neither the illumination nor the skipping metadata of the light operators, so none of these requests a recompute; the
    // Intensity and Octree renderers ignore them.
    bool SetLabelVolume(const uint8_t* Labels, size_t NumBytes)
    {
        return RaymarchResources.Handle && tbrm_upload_label_volume(RaymarchResources.Handle, Labels, NumBytes) == TBRM_OK;
    }
    bool UpdateLabelRegion(const int32_t Origin[3], const int32_t Extent[3], const uint8_t* Labels, size_t NumBytes)
    {
        return RaymarchResources.Handle && tbrm_update_label_region(RaymarchResources.Handle, Origin, Extent, Labels, NumBytes) == TBRM_OK;
    }
    bool SetLabelColors(const float* Rgba256x4)
    {
        return RaymarchResources.Handle && tbrm_set_label_colors(RaymarchResources.Handle, Rgba256x4) == TBRM_OK;
    }
    bool ClearLabelVolume() { return RaymarchResources.Handle && tbrm_release_label_volume(RaymarchResources.Handle) == TBRM_OK; }

    // Seeded region growing (include/tbrm_segment.h; no counterpart in the reference): the voxels with a stored value in [Lo, Hi]
    // connected to a seed (NumSeeds voxels x, y, z; none: every such voxel) get NewLabel (-1: measured only), on the device. Like
    // the other label edits it requests no recompute. A writing call attaches an empty label volume when none is attached.
    bool GrowRegion(const int32_t* SeedsXYZ, int NumSeeds, double Lo, double Hi, int NewLabel, int Connectivity, FGrowResult& Out,
                    bool bRelativeToSeed = false)
    {
        Out = FGrowResult{};
        if (!RaymarchResources.Handle) return false;
        if (NewLabel >= 0 && !tbrm_has_label_volume(RaymarchResources.Handle) && tbrm_attach_empty_label_volume(RaymarchResources.Handle) != TBRM_OK) return false;
        tbrm_grow_desc d{};
        d.connectivity = Connectivity;
        d.new_label = NewLabel;
        d.relative_to_seed = bRelativeToSeed ? 1 : 0;
        d.lo = Lo;
        d.hi = Hi;
        for (uint32_t& w : d.writable) w = 0xffffffffu;
        tbrm_grow_result r{};
        if (tbrm_grow_region(RaymarchResources.Handle, &d, SeedsXYZ, NumSeeds, &r) != TBRM_OK) return false;
        Out.Voxels = r.voxels;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; }
        Out.Passes = r.passes;
        Out.LoUsed = r.lo_used;
        Out.HiUsed = r.hi_used;
        return true;
    }
    // The click: the voxel the lit march first gets opaque at under pixel (Px, Py) (PickVolume's call, then tbrm_host_hit_voxel) and
    // from it every connected voxel whose stored value is within Tolerance of that voxel's. A ray that meets nothing grows nothing
    // (true, Out.bSeeded false).
    bool GrowRegionAt(const tbrm_camera& Camera, int Px, int Py, float Threshold, double Tolerance, int NewLabel, int Connectivity, FGrowResult& Out)
    {
        Out = FGrowResult{};
        if (!RaymarchResources.bIsInitialized) return false;
        const tbrm_raymarch_params rp{RaymarchingSteps, -1, 1, 0};
        const tbrm_world_params w = WorldParameters.abi();
        tbrm_hit h{};
        if (tbrm_pick(RaymarchResources.Handle, &Camera, Px, Py, &rp, &w, Threshold, &h, nullptr, nullptr) != TBRM_OK) return false;
        if (h.sample < 0) return true;
        const int32_t dims[3] = {RaymarchResources.SizeX, RaymarchResources.SizeY, RaymarchResources.SizeZ};
        int32_t seed[3] = {0, 0, 0};
        if (tbrm_host_hit_voxel(dims, &h, seed) != TBRM_OK) return false;
        const bool ok = GrowRegion(seed, 1, -Tolerance, Tolerance, NewLabel, Connectivity, Out, true);
        Out.bSeeded = true;
        for (int c = 0; c < 3; ++c) Out.Seed[c] = seed[c];
        return ok;
    }

    // Binary morphology of one label (include/tbrm_morphology.h; no counterpart in the reference): Op (TBRM_MORPH_DILATE .. CLOSE)
    // by Radius unit steps of the 6-neighbour cross or the 3 x 3 x 3 cube, on the device. Voxels that join get Label (over any
    // label), voxels that leave get EraseLabel; bMeasureOnly counts them and writes nothing. Like the other label edits it requests
    // no recompute. Needs a label volume.
    bool MorphLabel(int Op, int Radius, int Label, FMorphResult& Out, int Connectivity = 6, int EraseLabel = 0, bool bMeasureOnly = false)
    {
        Out = FMorphResult{};
        if (!RaymarchResources.Handle || Label < 0 || Label > 255) return false;
        tbrm_morph_desc d{};
        d.op = Op;
        d.radius = Radius;
        d.connectivity = Connectivity;
        d.new_label = bMeasureOnly ? -1 : Label;
        d.erase_label = EraseLabel;
        d.source[Label >> 5] = 1u << (Label & 31);
        for (uint32_t& w : d.writable) w = 0xffffffffu;
        tbrm_morph_result r{};
        if (tbrm_morph_labels(RaymarchResources.Handle, &d, &r) != TBRM_OK) return false;
        Out.SourceVoxels = r.source_voxels;
        Out.ResultVoxels = r.result_voxels;
        Out.Added = r.added;
        Out.Removed = r.removed;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; }
        Out.Launches = r.launches;
        return true;
    }
    bool DilateLabel(int Radius, int Label, FMorphResult& Out, int Connectivity = 6) { return MorphLabel(TBRM_MORPH_DILATE, Radius, Label, Out, Connectivity); }
    bool ErodeLabel(int Radius, int Label, FMorphResult& Out, int Connectivity = 6) { return MorphLabel(TBRM_MORPH_ERODE, Radius, Label, Out, Connectivity); }
    bool OpenLabel(int Radius, int Label, FMorphResult& Out, int Connectivity = 6) { return MorphLabel(TBRM_MORPH_OPEN, Radius, Label, Out, Connectivity); }
    bool CloseLabel(int Radius, int Label, FMorphResult& Out, int Connectivity = 6) { return MorphLabel(TBRM_MORPH_CLOSE, Radius, Label, Out, Connectivity); }

    // A Euclidean margin of one label (include/tbrm_margin.h; no counterpart in the reference): Op (TBRM_MARGIN_EXPAND .. CLOSE) by
    // RadiusWorld, a distance in the unit of VoxelSpacing (voxels when there is none), as a ball on the anisotropic grid, on the
    // device. Voxels that join get Label (over any label), voxels that leave get EraseLabel; bMeasureOnly counts them and writes
    // nothing. Like the other label edits it requests no recompute. Needs a label volume.
    bool MarginLabel(int Op, double RadiusWorld, int Label, FMarginResult& Out, int EraseLabel = 0, bool bMeasureOnly = false)
    {
        Out = FMarginResult{};
        if (!RaymarchResources.Handle || Label < 0 || Label > 255) return false;
        const bool unit = VoxelSpacing[0] == 0.0 && VoxelSpacing[1] == 0.0 && VoxelSpacing[2] == 0.0;
        const double spacing[3] = {unit ? 1.0 : VoxelSpacing[0], unit ? 1.0 : VoxelSpacing[1], unit ? 1.0 : VoxelSpacing[2]};
        tbrm_margin_desc d{};
        if (tbrm_host_margin_weights(spacing, RadiusWorld, d.weights, &d.limit) != TBRM_OK) return false;
        d.op = Op;
        d.new_label = bMeasureOnly ? -1 : Label;
        d.erase_label = EraseLabel;
        d.source[Label >> 5] = 1u << (Label & 31);
        for (uint32_t& w : d.writable) w = 0xffffffffu;
        tbrm_margin_result r{};
        if (tbrm_margin_labels(RaymarchResources.Handle, &d, &r) != TBRM_OK) return false;
        Out.SourceVoxels = r.source_voxels;
        Out.ResultVoxels = r.result_voxels;
        Out.Added = r.added;
        Out.Removed = r.removed;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; Out.Reach[c] = r.reach[c]; Out.Weights[c] = d.weights[c]; }
        Out.Limit = d.limit;
        Out.Launches = r.launches;
        return true;
    }
    bool ExpandLabelBy(double RadiusWorld, int Label, FMarginResult& Out) { return MarginLabel(TBRM_MARGIN_EXPAND, RadiusWorld, Label, Out); }
    bool ShrinkLabelBy(double RadiusWorld, int Label, FMarginResult& Out, int EraseLabel = 0) { return MarginLabel(TBRM_MARGIN_SHRINK, RadiusWorld, Label, Out, EraseLabel); }
    bool OpenLabelBy(double RadiusWorld, int Label, FMarginResult& Out, int EraseLabel = 0) { return MarginLabel(TBRM_MARGIN_OPEN, RadiusWorld, Label, Out, EraseLabel); }
    bool CloseLabelBy(double RadiusWorld, int Label, FMarginResult& Out, int EraseLabel = 0) { return MarginLabel(TBRM_MARGIN_CLOSE, RadiusWorld, Label, Out, EraseLabel); }

    // Smoothing of one label (include/tbrm_smooth.h; no counterpart in the reference): a voxel belongs to the label afterwards where
    // more than RankNum / RankDen of the box of RadiusInVolumeUnits round it — a distance in the unit of VoxelSpacing (voxels when
    // there is none), rounded to voxels per axis, the box clipped to the volume — does now; Iterations passes, on the device. Voxels
    // that join get Label (over any label), voxels that leave get EraseLabel; bMeasureOnly counts them and writes nothing. Like the
    // other label edits it requests no recompute. Needs a label volume.
    bool SmoothLabel(int Label, double RadiusInVolumeUnits, int Iterations, FSmoothResult& Out, int RankNum = 1, int RankDen = 2, int EraseLabel = 0,
                     bool bMeasureOnly = false)
    {
        Out = FSmoothResult{};
        if (!RaymarchResources.Handle || Label < 0 || Label > 255) return false;
        const bool unit = VoxelSpacing[0] == 0.0 && VoxelSpacing[1] == 0.0 && VoxelSpacing[2] == 0.0;
        const double spacing[3] = {unit ? 1.0 : VoxelSpacing[0], unit ? 1.0 : VoxelSpacing[1], unit ? 1.0 : VoxelSpacing[2]};
        tbrm_smooth_desc d{};
        if (tbrm_host_smooth_radii(spacing, RadiusInVolumeUnits, d.radius) != TBRM_OK) return false;
        d.rank_num = RankNum;
        d.rank_den = RankDen;
        d.iterations = Iterations;
        d.new_label = bMeasureOnly ? -1 : Label;
        d.erase_label = EraseLabel;
        d.source[Label >> 5] = 1u << (Label & 31);
        for (uint32_t& w : d.writable) w = 0xffffffffu;
        tbrm_smooth_result r{};
        if (tbrm_smooth_labels(RaymarchResources.Handle, &d, &r) != TBRM_OK) return false;
        Out.SourceVoxels = r.source_voxels;
        Out.ResultVoxels = r.result_voxels;
        Out.Added = r.added;
        Out.Removed = r.removed;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; Out.Radius[c] = d.radius[c]; Out.Reach[c] = r.reach[c]; }
        Out.Launches = r.launches;
        return true;
    }
    // the median: a strict majority of the box
    bool MedianLabel(int Label, double RadiusInVolumeUnits, int Iterations, FSmoothResult& Out) { return SmoothLabel(Label, RadiusInVolumeUnits, Iterations, Out, 1, 2); }

    // Scissors (include/tbrm_scissors.h; no counterpart in the reference): the lasso Polygon — x0, y0, x1, y1, .. in pixels of the view
    // Camera rendered, closed by itself, even-odd — cuts or fills Label in the voxels whose centre Camera sees under it between the
    // depths DepthMin and DepthMax along the camera's forward (world units: a hit's Depth; HUGE_VAL: no far limit), on the device. Op
    // is TBRM_SCISSORS_*: voxels that join get Label (over any label), voxels that leave get EraseLabel; bMeasureOnly counts them and
    // writes nothing. Like the other label edits it requests no recompute. Needs a label volume.
    bool ScissorLabel(const tbrm_camera& Camera, const std::vector<double>& Polygon, int Op, int Label, double DepthMin, double DepthMax, FScissorsResult& Out,
                      int EraseLabel = 0, bool bMeasureOnly = false)
    {
        Out = FScissorsResult{};
        if (!RaymarchResources.Handle || Label < 0 || Label > 255 || Polygon.size() < 6 || (Polygon.size() & 1)) return false;
        const tbrm_world_params w = WorldParameters.abi();
        const int32_t dims[3] = {RaymarchResources.SizeX, RaymarchResources.SizeY, RaymarchResources.SizeZ};
        tbrm_scissors_desc d{};
        if (tbrm_host_scissors_projection(dims, &w, &Camera, DepthMin, DepthMax, &d.projection) != TBRM_OK) return false;
        std::vector<uint32_t> Mask((size_t) ((Camera.width + 31) / 32) * (size_t) Camera.height);
        if (tbrm_host_scissors_polygon(Polygon.data(), Polygon.size() / 2, Camera.width, Camera.height, Mask.data(), Mask.size()) != TBRM_OK) return false;
        d.op = Op;
        d.new_label = bMeasureOnly ? -1 : Label;
        d.erase_label = EraseLabel;
        d.source[Label >> 5] = 1u << (Label & 31);
        for (uint32_t& m : d.writable) m = 0xffffffffu;
        tbrm_scissors_result r{};
        if (tbrm_scissors_labels(RaymarchResources.Handle, &d, Mask.data(), Mask.size(), &r) != TBRM_OK) return false;
        Out.SourceVoxels = r.source_voxels;
        Out.ResultVoxels = r.result_voxels;
        Out.Added = r.added;
        Out.Removed = r.removed;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; }
        Out.BricksInside = r.bricks_inside;
        Out.BricksOutside = r.bricks_outside;
        Out.BricksProjected = r.bricks_projected;
        Out.Launches = r.launches;
        for (uint32_t m : Mask)
            for (; m; m &= m - 1) ++Out.MaskPixels;
        return true;
    }
    // the three everyday cuts, through the whole depth of the view
    bool EraseInsideLasso(const tbrm_camera& Camera, const std::vector<double>& Polygon, int Label, FScissorsResult& Out) { return ScissorLabel(Camera, Polygon, TBRM_SCISSORS_ERASE_INSIDE, Label, 0.0, HUGE_VAL, Out); }
    bool KeepInsideLasso(const tbrm_camera& Camera, const std::vector<double>& Polygon, int Label, FScissorsResult& Out) { return ScissorLabel(Camera, Polygon, TBRM_SCISSORS_ERASE_OUTSIDE, Label, 0.0, HUGE_VAL, Out); }
    bool FillInsideLasso(const tbrm_camera& Camera, const std::vector<double>& Polygon, int Label, FScissorsResult& Out) { return ScissorLabel(Camera, Polygon, TBRM_SCISSORS_FILL_INSIDE, Label, 0.0, HUGE_VAL, Out); }

    // Grow from seeds (include/tbrm_compete.h; no counterpart in the reference): the voxels that hold one of SeedLabels compete for
    // the claimable voxels of the box, each of which goes to the label that reaches it at the least cost over face steps, on the
    // device. Like the other label edits it requests no recompute. Needs a label volume.
    // The step costs of a spacing: Finest along the axis of the smallest spacing, the others in proportion, rounded and clamped to
    // 1 .. 65535; unit spacing (VoxelSpacing all zero): Finest along every axis.
    void StepCostFromSpacing(int Finest, int Out[3]) const
    {
        const bool unit = VoxelSpacing[0] == 0.0 && VoxelSpacing[1] == 0.0 && VoxelSpacing[2] == 0.0;
        double least = HUGE_VAL;
        for (double s : VoxelSpacing)
            if (s > 0.0 && s < least) least = s;
        for (int c = 0; c < 3; ++c) {
            const double v = unit || !(VoxelSpacing[c] > 0.0) ? (double) Finest : std::floor((double) Finest * VoxelSpacing[c] / least + 0.5);
            Out[c] = v < 1.0 ? 1 : (v > (double) TBRM_COMPETE_MAX_STEP_COST ? TBRM_COMPETE_MAX_STEP_COST : (int) v);
        }
    }
    bool GrowFromSeeds(const std::vector<int>& SeedLabels, const FCompeteOptions& Options, FCompeteResult& Out, std::vector<uint32_t>* Costs = nullptr)
    {
        Out = FCompeteResult{};
        if (!RaymarchResources.Handle || SeedLabels.empty()) return false;
        tbrm_compete_desc d{};
        for (int c = 0; c < 3; ++c) { d.origin[c] = Options.Origin[c]; d.extent[c] = Options.Extent[c]; }
        d.connectivity = 6;
        d.measure_only = Options.bMeasureOnly ? 1 : 0;
        int fromSpacing[3];
        StepCostFromSpacing(Options.SpacingCost, fromSpacing);
        for (int c = 0; c < 3; ++c) Out.StepCost[c] = d.step_cost[c] = Options.StepCost[c] >= 0 ? Options.StepCost[c] : fromSpacing[c];
        d.value_shift = Options.ValueShift;
        d.cost_limit = Options.CostLimit;
        const bool isFloat = RaymarchResources.DataFormat == TBRM_FMT_R32_FLOAT;
        d.lo = Options.Lo;
        d.hi = Options.Hi;
        if (Options.Hi < Options.Lo) {
            d.lo = isFloat ? -3.4028234663852886e38 : 0.0;
            d.hi = isFloat ? 3.4028234663852886e38 : (RaymarchResources.DataFormat == TBRM_FMT_G8 ? 255.0 : 65535.0);
        }
        if (isFloat && tbrm_host_compete_float_range(Options.FloatLo, Options.FloatHi, &d.float_origin, &d.float_scale) != TBRM_OK) return false;
        for (int l : SeedLabels) {
            if (l < 0 || l > 255) return false;
            d.seeds[l >> 5] |= 1u << (l & 31);
        }
        if (Options.Writable.empty())
            for (uint32_t& w : d.writable) w = 0xffffffffu;
        for (int l : Options.Writable) {
            if (l < 0 || l > 255) return false;
            d.writable[l >> 5] |= 1u << (l & 31);
        }
        if (Costs) {
            const bool whole = d.extent[0] == 0 && d.extent[1] == 0 && d.extent[2] == 0;
            const size_t n = whole ? (size_t) RaymarchResources.SizeX * RaymarchResources.SizeY * RaymarchResources.SizeZ
                                   : (size_t) std::max(d.extent[0], 0) * (size_t) std::max(d.extent[1], 0) * (size_t) std::max(d.extent[2], 0);
            Costs->assign(n, TBRM_COMPETE_NO_COST);
        }
        tbrm_compete_result r{};
        if (tbrm_compete_labels(RaymarchResources.Handle, &d, Costs && !Costs->empty() ? Costs->data() : nullptr, &r) != TBRM_OK) return false;
        Out.SeedVoxels = r.seed_voxels;
        Out.Claimable = r.claimable;
        Out.Claimed = r.claimed;
        Out.Relabelled = r.relabelled;
        for (int l = 0; l < 256; ++l) Out.ClaimedPerLabel[l] = r.claimed_per_label[l];
        Out.MaxCost = r.max_cost;
        Out.Passes = r.passes;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; }
        return true;
    }

    // The paint brush (include/tbrm_paint.h; no counterpart in the reference): a stroke of capsules of RadiusWorld — a distance in the
    // unit of VoxelSpacing (voxels when there is none) — through Points (x0, y0, z0, x1, .. in eighths of a voxel: the centre of voxel i
    // is at 8 i; one point is a ball) is painted into Label (Op TBRM_PAINT_PAINT: voxels that join get Label) or erased from it
    // (TBRM_PAINT_ERASE: voxels that leave get Options.EraseTo), on the device, at the cost of the bricks the stroke touches. Like the
    // other label edits it requests no recompute. Needs a label volume.
    bool PaintStroke(int Op, const std::vector<int32_t>& Points, double RadiusWorld, int Label, FPaintResult& Out, const FPaintOptions& Options = FPaintOptions())
    {
        Out = FPaintResult{};
        if (!RaymarchResources.Handle || Label < 0 || Label > 255 || Points.empty() || Points.size() % 3) return false;
        const bool unit = VoxelSpacing[0] == 0.0 && VoxelSpacing[1] == 0.0 && VoxelSpacing[2] == 0.0;
        const double spacing[3] = {unit ? 1.0 : VoxelSpacing[0], unit ? 1.0 : VoxelSpacing[1], unit ? 1.0 : VoxelSpacing[2]};
        tbrm_paint_desc d{};
        if (tbrm_host_paint_brush(spacing, RadiusWorld, d.weights, &d.limit) != TBRM_OK) return false;
        for (int c = 0; c < 3; ++c) { d.origin[c] = Options.Origin[c]; d.extent[c] = Options.Extent[c]; }
        d.op = Op;
        d.new_label = Options.bMeasureOnly ? -1 : Label;
        d.erase_label = Options.EraseTo;
        d.gate = Options.bGate ? 1 : 0;
        d.lo = Options.Lo;
        d.hi = Options.Hi;
        d.source[Label >> 5] = 1u << (Label & 31);
        if (Options.Writable.empty())
            for (uint32_t& w : d.writable) w = 0xffffffffu;
        for (int l : Options.Writable) {
            if (l < 0 || l > 255) return false;
            d.writable[l >> 5] |= 1u << (l & 31);
        }
        tbrm_paint_result r{};
        if (tbrm_paint_labels(RaymarchResources.Handle, &d, Points.data(), Points.size() / 3, &r) != TBRM_OK) return false;
        Out.StampVoxels = r.stamp_voxels;
        Out.Added = r.added;
        Out.Removed = r.removed;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; Out.Weights[c] = d.weights[c]; }
        Out.Points = (int) (Points.size() / 3);
        Out.Segments = r.segments;
        Out.BricksWhole = r.bricks_whole;
        Out.BricksUntouched = r.bricks_untouched;
        Out.BricksEvaluated = r.bricks_evaluated;
        Out.Launches = r.launches;
        Out.Limit = d.limit;
        return true;
    }
    bool PaintLabel(const std::vector<int32_t>& Points, double RadiusWorld, int Label, FPaintResult& Out, const FPaintOptions& Options = FPaintOptions())
    {
        return PaintStroke(TBRM_PAINT_PAINT, Points, RadiusWorld, Label, Out, Options);
    }
    bool EraseLabel(const std::vector<int32_t>& Points, double RadiusWorld, int Label, FPaintResult& Out, const FPaintOptions& Options = FPaintOptions())
    {
        return PaintStroke(TBRM_PAINT_ERASE, Points, RadiusWorld, Label, Out, Options);
    }
    // A stroke along picked points of the rendered surface: the hits of Hits (PickVolume; records without a hit are passed over) in
    // their order become the stroke's points (tbrm_host_paint_stroke: quantised to eighths of a voxel, repeats dropped, long segments
    // split). No hit among them: false.
    bool PaintAlongHits(const std::vector<FVolumeHit>& Hits, double RadiusWorld, int Label, FPaintResult& Out, int Op = TBRM_PAINT_PAINT,
                        const FPaintOptions& Options = FPaintOptions())
    {
        Out = FPaintResult{};
        if (!RaymarchResources.Handle) return false;
        std::vector<float> Uvw;
        for (const FVolumeHit& h : Hits)
            if (h.bHit) Uvw.insert(Uvw.end(), h.Uvw, h.Uvw + 3);
        if (Uvw.empty()) return false;
        const bool unit = VoxelSpacing[0] == 0.0 && VoxelSpacing[1] == 0.0 && VoxelSpacing[2] == 0.0;
        const double spacing[3] = {unit ? 1.0 : VoxelSpacing[0], unit ? 1.0 : VoxelSpacing[1], unit ? 1.0 : VoxelSpacing[2]};
        uint32_t weights[3], limit = 0;
        if (tbrm_host_paint_brush(spacing, RadiusWorld, weights, &limit) != TBRM_OK) return false;
        const int32_t dims[3] = {RaymarchResources.SizeX, RaymarchResources.SizeY, RaymarchResources.SizeZ};
        size_t n = 0;
        tbrm_host_paint_stroke(dims, Uvw.data(), Uvw.size() / 3, weights, nullptr, 0, &n); // (how many points: the call itself says "too small")
        if (n == 0) return false;
        std::vector<int32_t> Points(3 * n);
        if (tbrm_host_paint_stroke(dims, Uvw.data(), Uvw.size() / 3, weights, Points.data(), n, &n) != TBRM_OK) return false;
        return PaintStroke(Op, Points, RadiusWorld, Label, Out, Options);
    }

    // The surface of Label as an indexed triangle mesh (include/tbrm_surface.h; the reference's closed surfaces are surface nets on the
    // binary label map too): extracted on the device, one vertex per cell of 2 x 2 x 2 voxels the label's boundary passes through.
    // Positions are in the volume's local unit cube — the space the hit maps' Uvw live in — so the actor's transform places the mesh
    // where the volume is rendered. Origin / Extent cut the label to a box (all-zero extent: the whole volume); the surface is closed
    // at the box's faces. A read: it changes no label and requests no recompute. Needs a label volume.
    bool SurfaceDesc(int Label, const int Origin[3], const int Extent[3], tbrm_surface_desc& d) const
    {
        if (!RaymarchResources.Handle || Label < 0 || Label > 255) return false;
        d = tbrm_surface_desc{};
        for (int c = 0; c < 3; ++c) { d.origin[c] = Origin && Extent ? Origin[c] : 0; d.extent[c] = Extent ? Extent[c] : 0; }
        d.source[Label >> 5] = 1u << (Label & 31);
        const int32_t dims[3] = {RaymarchResources.SizeX, RaymarchResources.SizeY, RaymarchResources.SizeZ};
        return tbrm_host_surface_unit_cube(dims, d.scale, d.offset) == TBRM_OK;
    }
    static void SurfaceCounts(const tbrm_surface_result& r, FLabelSurface& Out)
    {
        Out.SetVoxels = r.set_voxels;
        Out.Vertices = r.vertices;
        Out.Quads = r.quads;
        for (int c = 0; c < 3; ++c) { Out.QuadsAxis[c] = r.quads_axis[c]; Out.CellMin[c] = r.cell_min[c]; Out.CellMax[c] = r.cell_max[c]; }
        Out.BlocksEvaluated = r.blocks_evaluated;
        Out.BlocksSkipped = r.blocks_skipped;
        Out.Launches = r.launches;
    }
    bool MeasureLabelSurface(int Label, FLabelSurface& Out, const int Origin[3] = nullptr, const int Extent[3] = nullptr)
    {
        Out = FLabelSurface{};
        tbrm_surface_desc d{};
        if (!SurfaceDesc(Label, Origin, Extent, d)) return false;
        d.flags = TBRM_SURFACE_MEASURE;
        tbrm_surface_result r{};
        if (tbrm_label_surface(RaymarchResources.Handle, &d, nullptr, nullptr, nullptr, &r) != TBRM_OK) return false;
        SurfaceCounts(r, Out);
        return true;
    }
    bool ExtractLabelSurface(int Label, FLabelSurface& Out, const int Origin[3] = nullptr, const int Extent[3] = nullptr)
    {
        if (!MeasureLabelSurface(Label, Out, Origin, Extent)) return false;
        tbrm_surface_desc d{};
        SurfaceDesc(Label, Origin, Extent, d);
        d.flags = TBRM_SURFACE_TRIANGLES;
        d.vertex_capacity = Out.Vertices;
        d.quad_capacity = Out.Quads;
        Out.Records.resize((size_t) Out.Vertices);
        Out.Positions.resize(3 * (size_t) Out.Vertices);
        Out.Triangles.resize(6 * (size_t) Out.Quads);
        tbrm_surface_result r{};
        if (tbrm_label_surface(RaymarchResources.Handle, &d, Out.Records.data(), Out.Triangles.data(), Out.Positions.data(), &r) != TBRM_OK) {
            Out = FLabelSurface{};
            return false;
        }
        SurfaceCounts(r, Out);
        // the gradient of an indicator on voxels of unequal spacing: each component over its spacing
        const bool unit = VoxelSpacing[0] == 0.0 && VoxelSpacing[1] == 0.0 && VoxelSpacing[2] == 0.0;
        Out.Normals.resize(3 * (size_t) Out.Vertices);
        for (size_t i = 0; i < Out.Records.size(); ++i) {
            double n[3], len = 0.0;
            for (int c = 0; c < 3; ++c) {
                n[c] = (double) Out.Records[i].normal[c] / (unit ? 1.0 : VoxelSpacing[c]);
                len += n[c] * n[c];
            }
            len = std::sqrt(len);
            for (int c = 0; c < 3; ++c) Out.Normals[3 * i + c] = len > 0.0 ? (float) (n[c] / len) : 0.0f;
        }
        return true;
    }

    // The islands of one label (include/tbrm_islands.h; no counterpart in the reference): its connected components, ordered by size,
    // on the device. The four tools are parameter sets of one rule. Like the other label edits they request no recompute. They need a
    // label volume.
    bool LabelIslands(const tbrm_islands_desc& Desc, FIslandsResult& Out, tbrm_island* Table = nullptr, int Capacity = 0)
    {
        Out = FIslandsResult{};
        if (!RaymarchResources.Handle) return false;
        tbrm_islands_result r{};
        if (tbrm_label_islands(RaymarchResources.Handle, &Desc, Table, Capacity, &r) != TBRM_OK) return false;
        Out.SetVoxels = r.set_voxels;
        Out.Islands = r.islands;
        Out.Spared = r.spared;
        Out.Kept = r.kept;
        Out.Dropped = r.dropped;
        Out.KeptVoxels = r.kept_voxels;
        Out.DroppedVoxels = r.dropped_voxels;
        Out.Largest = r.largest;
        Out.Relabelled = r.relabelled;
        for (int c = 0; c < 3; ++c) { Out.BoxMin[c] = r.bbox_min[c]; Out.BoxMax[c] = r.bbox_max[c]; }
        return true;
    }
    // the Count largest islands of Label stay, the others get EraseLabel
    bool KeepLargestIslands(int Label, int Count, FIslandsResult& Out, int Connectivity = 6, int EraseLabel = 0)
    {
        Out = FIslandsResult{};
        if (Label < 0 || Label > 255 || Count < 1) return false;
        tbrm_islands_desc d = IslandsOf(Label, Connectivity);
        d.max_islands = Count;
        d.drop_label = EraseLabel;
        return LabelIslands(d, Out);
    }
    // islands of Label with fewer than MinVoxels voxels get EraseLabel
    bool RemoveSmallIslands(int Label, uint64_t MinVoxels, FIslandsResult& Out, int Connectivity = 6, int EraseLabel = 0)
    {
        Out = FIslandsResult{};
        if (Label < 0 || Label > 255) return false;
        tbrm_islands_desc d = IslandsOf(Label, Connectivity);
        d.min_voxels = MinVoxels;
        d.drop_label = EraseLabel;
        return LabelIslands(d, Out);
    }
    // the MaxIslands largest islands of Label get FirstLabel, FirstLabel + 1, ..; the others DropLabel (-1: they stay as they are)
    bool SplitIslands(int Label, int FirstLabel, int MaxIslands, FIslandsResult& Out, int Connectivity = 6, int DropLabel = -1)
    {
        Out = FIslandsResult{};
        if (Label < 0 || Label > 255) return false;
        tbrm_islands_desc d = IslandsOf(Label, Connectivity);
        d.max_islands = MaxIslands;
        d.keep_label = FirstLabel;
        d.label_step = 1;
        d.drop_label = DropLabel;
        return LabelIslands(d, Out);
    }
    // what Label encloses — the islands of every other label that touch no face of the volume, of at most MaxVoxels voxels
    // (UINT64_MAX: of any size) — gets Label; Connectivity is that of the enclosed background
    bool FillLabelHoles(int Label, FIslandsResult& Out, uint64_t MaxVoxels = UINT64_MAX, int Connectivity = 6)
    {
        Out = FIslandsResult{};
        if (Label < 0 || Label > 255) return false;
        tbrm_islands_desc d = IslandsOf(Label, Connectivity);
        for (uint32_t& w : d.source) w = ~w;
        d.spare_border = 1;
        d.min_voxels = MaxVoxels == UINT64_MAX ? UINT64_MAX : MaxVoxels + 1;
        d.drop_label = Label;
        return LabelIslands(d, Out);
    }

    // :746-784 — every windowing change requests a full recompute
    void SetWindowCenter(float Center) { if (Center != RaymarchResources.WindowingParameters.Center) { RaymarchResources.WindowingParameters.Center = Center; WindowingChanged(); } }
    void SetWindowWidth(float Width) { if (Width != RaymarchResources.WindowingParameters.Width) { RaymarchResources.WindowingParameters.Width = Width; WindowingChanged(); } }
    void SetLowCutoff(bool Cutoff) { if (Cutoff != RaymarchResources.WindowingParameters.LowCutoff) { RaymarchResources.WindowingParameters.LowCutoff = Cutoff; WindowingChanged(); } }
    void SetHighCutoff(bool Cutoff) { if (Cutoff != RaymarchResources.WindowingParameters.HighCutoff) { RaymarchResources.WindowingParameters.HighCutoff = Cutoff; WindowingChanged(); } }
    void SetRaymarchSteps(float InSteps) { RaymarchingSteps = InSteps; } // :802-819
    void SwitchRenderer(ERaymarchMaterial InSelectRaymarchMaterial) // :786-800, :304-307
    {
        SelectRaymarchMaterial = InSelectRaymarchMaterial;
        if (InSelectRaymarchMaterial == ERaymarchMaterial::Lit) bRequestedRecompute = true;
        if (InSelectRaymarchMaterial == ERaymarchMaterial::Octree) bRequestedOctreeRebuild = true;
    }

    FRaymarchWorldParameters GetWorldParameters() const // :630-646
    {
        FRaymarchWorldParameters r;
        if (ClippingPlane) r.ClippingPlaneParameters = ClippingPlane->GetCurrentParameters();
        else { r.ClippingPlaneParameters.Center = FVector{0, 0, 100000}; r.ClippingPlaneParameters.Direction = FVector{0, 0, -1}; }
        r.VolumeTransform = ComponentTransform;
        return r;
    }

    void Tick(float /*DeltaTime*/) // :327-416
    {
        if (!RaymarchResources.bIsInitialized || !bVisible) return;
        if (WorldParameters != GetWorldParameters()) { // volume transform changed or clipping plane moved
            bRequestedRecompute = true;
            WorldParameters = GetWorldParameters();
        }
        if (bRequestedOctreeRebuild && SelectRaymarchMaterial == ERaymarchMaterial::Octree) { // :358-363
            URaymarchUtils::GenerateOctree(RaymarchResources);
            bRequestedOctreeRebuild = false; // also when generation failed, as in the reference: no retry every tick
        }
        if (SelectRaymarchMaterial != ERaymarchMaterial::Lit) return;
        if (bRequestedRecompute) { ResetAllLights(); return; }
        std::vector<ARaymarchLight*> LightsToUpdate;
        for (ARaymarchLight* Light : LightsArray) {
            if (!Light) continue;
            auto it = LightParametersMap.find(Light);
            if (it == LightParametersMap.end()) { LightParametersMap[Light] = Light->GetCurrentParameters(); LightsToUpdate.push_back(Light); }
            else if (Light->GetCurrentParameters() != it->second) LightsToUpdate.push_back(Light);
        }
        // more than half of the lights need an update -> a full reset is quicker (:400-404)
        if (LightsToUpdate.size() > 1 && LightsToUpdate.size() >= LightsArray.size() / 2) ResetAllLights();
        else
            for (ARaymarchLight* UpdatedLight : LightsToUpdate) {
                UpdateSingleLight(UpdatedLight);
                LightParametersMap[UpdatedLight] = UpdatedLight->GetCurrentParameters();
            }
    }

    void ResetAllLights() // :418-451
    {
        if (!RaymarchResources.bIsInitialized) return;
        ReserveForLights(); // (lights added since the resources were initialised)
        URaymarchUtils::ClearResourceLightVolumes(RaymarchResources, 0);
        ++Stats.Resets;
        bool bResetWasSuccessful = true;
        if (bBatchLightsOnReset && !ColoredHandle()) {
            std::vector<FDirLightParameters> All;
            for (ARaymarchLight* Light : LightsArray)
                if (Light) All.push_back(Light->GetCurrentParameters());
            URaymarchUtils::AddDirLightsToSingleVolume(RaymarchResources, All, true, WorldParameters, bResetWasSuccessful);
            Stats.LightAdds += (int) All.size();
            if (!bResetWasSuccessful) { std::fprintf(stderr, "Error. Could not add the lights.\n"); return; }
            if (bRecordLightsOnReset)
                for (ARaymarchLight* Light : LightsArray)
                    if (Light) LightParametersMap[Light] = Light->GetCurrentParameters();
            bRequestedRecompute = false;
            return;
        }
        for (ARaymarchLight* Light : LightsArray) {
            if (!Light) continue;
            if (ColoredHandle()) URaymarchUtils::AddColorDirLightToSingleVolume(RaymarchResources, Light->GetCurrentParameters(), true, WorldParameters, bResetWasSuccessful);
            else URaymarchUtils::AddDirLightToSingleVolume(RaymarchResources, Light->GetCurrentParameters(), true, WorldParameters, bResetWasSuccessful, bFastShader);
            ++Stats.LightAdds;
            if (!bResetWasSuccessful) { std::fprintf(stderr, "Error. Could not add/remove light %s.\n", Light->Name.c_str()); return; }
            // The reference leaves LightParametersMap untouched here (:418-451): a light that moved before a reset is
            // "changed" again on the next tick, from parameters that were never added to the volume. That behaviour is
            // kept by default; bRecordLightsOnReset makes the map follow the light volume's actual content instead.
            if (bRecordLightsOnReset) LightParametersMap[Light] = Light->GetCurrentParameters();
        }
        bRequestedRecompute = false;
    }

    void UpdateSingleLight(ARaymarchLight* UpdatedLight) // :453-465
    {
        bool bLightAddWasSuccessful = false;
        if (ColoredHandle()) URaymarchUtils::ChangeColorDirLightInSingleVolume(RaymarchResources, LightParametersMap[UpdatedLight], UpdatedLight->GetCurrentParameters(), WorldParameters, bLightAddWasSuccessful);
        else URaymarchUtils::ChangeDirLightInSingleVolume(RaymarchResources, LightParametersMap[UpdatedLight], UpdatedLight->GetCurrentParameters(), WorldParameters, bLightAddWasSuccessful);
        ++Stats.LightChanges;
        if (!bLightAddWasSuccessful) std::fprintf(stderr, "Error. Could not change light %s.\n", UpdatedLight->Name.c_str());
    }

    // Offscreen replacement of the M_Raymarch material pass: premultiplied RGBA float, Camera.width x Camera.height.
    bool RenderLit(const tbrm_camera& Camera, float* OutRGBA, int JitterFrame = -1, bool bSkipEmptySpace = true)
    {
        if (!RaymarchResources.bIsInitialized) return false;
        const tbrm_tile tile{0, 0, Camera.width, Camera.height, 1, 0};
        const tbrm_raymarch_params rp{RaymarchingSteps, JitterFrame, bSkipEmptySpace ? 1 : 0, 0};
        const tbrm_world_params w = WorldParameters.abi();
        ++Stats.Frames;
        return tbrm_raymarch_lit(RaymarchResources.Handle, &Camera, &tile, &rp, &w, OutRGBA) == TBRM_OK;
    }

    // Offscreen replacement of the M_Intensity_Raymarch material pass (the slice view, RaymarchVolume.cpp:72-73,:122-128).
    bool RenderIntensity(const tbrm_camera& Camera, float* OutRGBA, int JitterFrame = -1)
    {
        if (!RaymarchResources.Handle) return false;
        const tbrm_tile tile{0, 0, Camera.width, Camera.height, 1, 0};
        const tbrm_raymarch_params rp{RaymarchingSteps, JitterFrame, 0, 0};
        const tbrm_world_params w = WorldParameters.abi();
        ++Stats.Frames;
        return tbrm_raymarch_intensity(RaymarchResources.Handle, &Camera, &tile, &rp, &w, OutRGBA) == TBRM_OK;
    }

    // Offscreen replacement of the M_Octree_Raymarch material pass over level OctreeVolumeMip. Tick rebuilds the pyramid
    // when a rebuild was requested (new volume, SwitchRenderer(Octree); :358-363); a host that renders without ticking
    // gets the pending rebuild here.
    int OctreeVolumeMip = 0; // RaymarchVolume.h: the level the octree material samples
    bool bRequestedOctreeRebuild = true;
    bool RenderOctree(const tbrm_camera& Camera, float* OutRGBA, int JitterFrame = -1)
    {
        if (!RaymarchResources.Handle) return false;
        if (bRequestedOctreeRebuild) {
            if (!URaymarchUtils::GenerateOctree(RaymarchResources)) return false;
            bRequestedOctreeRebuild = false;
        }
        const tbrm_tile tile{0, 0, Camera.width, Camera.height, 1, 0};
        const tbrm_raymarch_params rp{RaymarchingSteps, JitterFrame, 0, 0};
        const tbrm_world_params w = WorldParameters.abi();
        ++Stats.Frames;
        return tbrm_raymarch_octree(RaymarchResources.Handle, &Camera, &tile, &rp, &w, OctreeVolumeMip, OutRGBA) == TBRM_OK;
    }

    // Picking and depth (include/tbrm_hit.h): what the lit march of this volume — current window, transfer function, clip plane,
    // labels and step count, no jitter — first gets opaque at, where "opaque" is an accumulated opacity above Threshold (0 .. 0.95).
    // Neither call touches the illumination or counts as a frame.
    bool PickVolume(const tbrm_camera& Camera, int Px, int Py, float Threshold, FVolumeHit& Out)
    {
        Out = FVolumeHit{};
        if (!RaymarchResources.bIsInitialized) return false;
        const tbrm_raymarch_params rp{RaymarchingSteps, -1, 1, 0};
        const tbrm_world_params w = WorldParameters.abi();
        tbrm_hit h{};
        double xyz[3] = {0, 0, 0};
        if (tbrm_pick(RaymarchResources.Handle, &Camera, Px, Py, &rp, &w, Threshold, &h, xyz, &Out.Depth) != TBRM_OK) return false;
        Out.bHit = h.sample >= 0;
        Out.WorldPosition = FVector{xyz[0], xyz[1], xyz[2]};
        Out.Value = h.value;
        Out.Label = h.label;
        Out.Sample = h.sample;
        for (int c = 0; c < 3; ++c) Out.Uvw[c] = h.uvw[c];
        return true;
    }
    // The visible surface as a depth buffer, Camera.width x Camera.height floats in the convention of the march's own scene depth
    // (+inf where a ray meets nothing): what scene geometry is composited against.
    bool RenderHitDepth(const tbrm_camera& Camera, float* OutDepth, float Threshold)
    {
        if (!RaymarchResources.bIsInitialized || !OutDepth) return false;
        const tbrm_tile tile{0, 0, Camera.width, Camera.height, 1, 0};
        const tbrm_raymarch_params rp{RaymarchingSteps, -1, 1, 0};
        const tbrm_world_params w = WorldParameters.abi();
        std::vector<tbrm_hit> Hits((size_t) (Camera.width > 0 ? Camera.width : 0) * (size_t) (Camera.height > 0 ? Camera.height : 0));
        return tbrm_raymarch_hits(RaymarchResources.Handle, &Camera, &tile, &rp, &w, Threshold, Hits.data(), OutDepth) == TBRM_OK;
    }

    // What the cube mesh would show with the currently selected material (SwitchRenderer, :786-800).
    bool Render(const tbrm_camera& Camera, float* OutRGBA, int JitterFrame = -1)
    {
        switch (SelectRaymarchMaterial) {
            case ERaymarchMaterial::Intensity: return RenderIntensity(Camera, OutRGBA, JitterFrame);
            case ERaymarchMaterial::Octree: return RenderOctree(Camera, OutRGBA, JitterFrame);
            default: return RenderLit(Camera, OutRGBA, JitterFrame);
        }
    }

    void FreeRaymarchResources() // :922-949
    {
        if (RaymarchResources.Handle) tbrm_resources_destroy(RaymarchResources.Handle);
        RaymarchResources.Handle = nullptr;
        RaymarchResources.bIsInitialized = false;
        bHasTF = false;
    }

private:
    std::map<ARaymarchLight*, FDirLightParameters> LightParametersMap;
    bool bHasTF = false;
    // the islands of one label, nothing written yet: every island kept, every byte left
    static tbrm_islands_desc IslandsOf(int Label, int Connectivity)
    {
        tbrm_islands_desc d{};
        d.connectivity = Connectivity;
        d.keep_label = -1;
        d.drop_label = -1;
        d.source[Label >> 5] = 1u << (Label & 31);
        return d;
    }
    // the histogram of ComputeHistogram and the value range [Lo, Hi] its bins cover (stored units)
    bool HistogramWithRange(int NumBins, std::vector<uint64_t>& Out, double& Lo, double& Hi)
    {
        Out.clear();
        if (!RaymarchResources.Handle || NumBins < 1 || NumBins > TBRM_HISTOGRAM_MAX_BINS) return false;
        tbrm_histogram_desc d{};
        d.n_bins = NumBins;
        if (RaymarchResources.DataFormat == TBRM_FMT_R32_FLOAT) {
            std::vector<tbrm_label_stat> Stats;
            if (!GetLabelStatistics(Stats)) return false;
            Lo = INFINITY; Hi = -INFINITY;
            for (const tbrm_label_stat& s : Stats) { Lo = std::min(Lo, s.min); Hi = std::max(Hi, s.max); }
            if (!std::isfinite(Lo) || !std::isfinite(Hi)) return false; // no finite voxel, or infinite ones: no range to bin
            if (!(Lo < Hi)) Hi = (double) std::nextafter((float) Lo, INFINITY); // a constant volume: one value wide
        } else { Lo = 0.0; Hi = RaymarchResources.DataFormat == TBRM_FMT_G8 ? 255.0 : 65535.0; }
        d.lo = Lo;
        d.hi = Hi;
        Out.assign((size_t) NumBins, 0);
        uint64_t Tally[4] = {0, 0, 0, 0};
        if (tbrm_volume_histogram(RaymarchResources.Handle, &d, Out.data(), Tally) == TBRM_OK) return true;
        Out.clear();
        return false;
    }
    bool ColoredHandle() const { return RaymarchResources.Handle && tbrm_resources_light_channels(RaymarchResources.Handle) == 3; }

    void InitializeRaymarchResources(int X, int Y, int Z, int Format) // :821-920
    {
        if (RaymarchResources.Handle) FreeRaymarchResources();
        tbrm_resources_desc d{};
        d.dim_x = X; d.dim_y = Y; d.dim_z = Z;
        d.data_format = Format;
        d.light_volume_32bit = bLightVolume32Bit ? 1 : 0;
        d.light_volume_half_resolution = RaymarchResources.LightVolumeHalfResolution ? 1 : 0;
        d.device = Device;
        d.data_address_mode = DataAddressMode;
        d.border_mode = TBRM_BORDER_ENGINE_8BIT;
        if ((bColoredLights ? tbrm_resources_create_rgb(&d, &RaymarchResources.Handle) : tbrm_resources_create(&d, &RaymarchResources.Handle)) != TBRM_OK) {
            std::fprintf(stderr, "Tried to initialize Raymarch resources: %s\n", tbrm_last_error());
            RaymarchResources.Handle = nullptr;
            return;
        }
        RaymarchResources.SizeX = X; RaymarchResources.SizeY = Y; RaymarchResources.SizeZ = Z;
        RaymarchResources.DataFormat = Format;
        ReservedLights = 0;
        ReserveForLights();
    }
    // Every buffer the light operators will need, now (:821-920 creates the read / write buffers and the light volume here, never
    // inside AddDirLightToSingleVolume): tbrm_resources_reserve for the lights the actor holds, four at least; again when more arrive.
    int ReservedLights = 0;
    void ReserveForLights()
    {
        if (!RaymarchResources.Handle) return;
        const int Want = std::max<int>(4, (int) LightsArray.size());
        if (Want <= ReservedLights) return;
        if (tbrm_resources_reserve(RaymarchResources.Handle, Want, 0) == TBRM_OK) ReservedLights = Want;
        else std::fprintf(stderr, "tbrm_resources_reserve: %s\n", tbrm_last_error());
    }
    void WindowingChanged()
    {
        if (RaymarchResources.Handle) { tbrm_windowing_params w = RaymarchResources.WindowingParameters.abi(); tbrm_set_windowing(RaymarchResources.Handle, &w); }
        bRequestedRecompute = true;
    }
};
using URaymarchVolume = ARaymarchVolume;

} // namespace tbrm_plugin
