// render_mhd — the drop-in path end to end, as a host without the engine would use it: MetaImage volume in
// (include/tbrm_volume_io.hpp, the reference's UMHDLoader + normalisation), two directional lights and a clip-free frame
// through the reference-named C++ host side (include/tbrm_plugin.hpp: ARaymarchVolume, ARaymarchLight, Tick), image out as
// binary PPM (premultiplied RGBA composited over black).
//
//   g++ -std=c++17 -O2 -I include examples/render_mhd.cpp -o render_mhd -L tbraymarcherplugin_amd/lib -ltbrm -lz
//       (plus -Wl,-rpath,$PWD/tbraymarcherplugin_amd/lib -Wl,-rpath,/opt/rocm/lib to run it in place)
//   ./render_mhd volume.mhd out.ppm [width height steps] [--light-color r,g,b] [--auto-window[=LOW,HIGH]] [--pick X,Y] [--grow X,Y,TOL[,LABEL]] [--morph OP,R[,LABEL]] [--margin OP,RADIUS[,LABEL]] [--smooth RADIUS[,ITERATIONS[,LABEL]]] [--islands OP,N[,LABEL]] [--scissors OP,LABEL,x0,y0,x1,y1,x2,y2[,..]] [--compete COST,SHIFT,LIMIT,LABEL@X,Y,Z,R[,LABEL@X,Y,Z,R..]] [--paint LABEL,RADIUS@X,Y,Z[;X,Y,Z..]] [--surface LABEL,FILE.obj]
//       --light-color: the key light's colour (components in [0, 1]) on an RGB light volume (include/tbrm_color_lights.h); the fill stays white
//       --auto-window: the window comes from the data (ARaymarchVolume::AutoWindow, include/tbrm_volume_stats.h): the span between
//                      the LOW and HIGH percentiles of the value histogram, 0.01,0.99 when not given
//       --pick: what the frame's pixel (X, Y) shows first (ARaymarchVolume::PickVolume, include/tbrm_hit.h): the spot where the ray's
//                      accumulated opacity passes 0.5, printed as one "pick" line
//       --grow: a click on the frame's pixel (X, Y) (ARaymarchVolume::GrowRegionAt, include/tbrm_segment.h): the voxels connected to the
//                      one under it whose stored value (the 16-bit code) is within TOL of its own get label LABEL (1 when not given)
//                      and the frame shows them in the label's colour; printed as one "grow" line with the label's mean value
//       --morph: after --grow, binary morphology of label LABEL (the grown label when not given) (ARaymarchVolume::MorphLabel,
//                      include/tbrm_morphology.h): OP is dilate, erode, open or close, R the radius in unit steps of the 6-neighbour
//                      cross; voxels that leave the label get label 0; printed as one "morph" line
//       --margin: after --grow and --morph, a Euclidean margin of label LABEL (the grown label when not given) (ARaymarchVolume::MarginLabel,
//                      include/tbrm_margin.h): OP is expand, shrink, open or close, RADIUS a distance in the units of the file's
//                      ElementSpacing — a ball on the anisotropic grid; voxels that leave the label get label 0; printed as one
//                      "margin" line
//       --smooth: after --grow, --morph and --margin, the median of label LABEL (the grown label when not given) (ARaymarchVolume::MedianLabel,
//                      include/tbrm_smooth.h): a voxel keeps or gets the label where a strict majority of the box of RADIUS round it —
//                      a distance in the units of the file's ElementSpacing, rounded to voxels per axis — has it; ITERATIONS passes
//                      (1 when not given); voxels that leave the label get label 0; printed as one "smooth" line
//       --scissors: after every other edit, the lasso through the points (x, y) — pixels of the rendered view, closed by itself, even-odd —
//                      cuts or fills label LABEL in the voxels the view sees under it, through its whole depth (ARaymarchVolume::ScissorLabel,
//                      include/tbrm_scissors.h): OP is erase_inside, erase_outside (keep only what is under the lasso), fill_inside or
//                      fill_outside; voxels that leave the label get label 0; printed as one "scissors" line
//       --compete: after every other edit, grow from seeds (ARaymarchVolume::GrowFromSeeds, include/tbrm_compete.h): a ball of R voxels
//                      round the voxel (X, Y, Z) is painted with LABEL for every LABEL@X,Y,Z,R, then the painted labels compete for every
//                      other voxel: a step costs COST along the axis of the file's finest ElementSpacing (the others in proportion) plus
//                      the difference of the two voxels' 16-bit codes >> SHIFT, up to the cost LIMIT (0: no limit); printed as one
//                      "compete" line
//       --surface: after every edit, the surface of label LABEL as a triangle mesh (ARaymarchVolume::ExtractLabelSurface,
//                      include/tbrm_surface.h) written to FILE.obj as a Wavefront OBJ: positions in the units of the file's ElementSpacing
//                      (voxels when it has none), one normal per vertex; printed as one "surface" line
//       --paint: after every other edit, a brush stroke (ARaymarchVolume::PaintLabel, include/tbrm_paint.h): capsules of RADIUS — a
//                      distance in the units of the file's ElementSpacing — through the points (X, Y, Z), voxels that need not be whole
//                      (rounded to eighths) nor inside the volume, are painted with LABEL over whatever is there; one point is a ball; an
//                      empty label volume is attached when there is none; printed as one "paint" line
//       --islands: after --grow, --morph, --margin and --smooth, the islands of label LABEL (the grown label when not given) (ARaymarchVolume::KeepLargestIslands
//                      and its kin, include/tbrm_islands.h), 6-connected: OP is keep (the N largest stay, the others get label 0), remove
//                      (islands of fewer than N voxels get label 0), split (the N largest get LABEL, LABEL + 1, ..) or fill (what the
//                      label encloses, up to N voxels a hole, 0: of any size, joins it); printed as one "islands" line
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tbrm_volume_io.hpp" // includes tbrm_plugin.hpp

using namespace tbrm_plugin;

int main(int argc, char** argv)
{
    float key_color[3] = {1.0f, 1.0f, 1.0f};
    bool colored = false, auto_window = false;
    float auto_low = 0.01f, auto_high = 0.99f;
    for (int i = 1; i < argc; ++i) // --auto-window[=LOW,HIGH] is one word
        if (!std::strncmp(argv[i], "--auto-window", 13)) {
            if (argv[i][13] == '=' ? std::sscanf(argv[i] + 14, "%f,%f", &auto_low, &auto_high) != 2 : argv[i][13] != 0) { argc = 0; break; }
            auto_window = true;
            for (int k = i; k + 1 < argc; ++k) argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    int pick_x = -1, pick_y = -1;
    bool pick = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--pick")) {
            if (std::sscanf(argv[i + 1], "%d,%d", &pick_x, &pick_y) != 2) { argc = 0; break; }
            pick = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    int grow_x = -1, grow_y = -1, grow_label = 1;
    double grow_tol = 0.0;
    bool grow = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--grow")) {
            if (std::sscanf(argv[i + 1], "%d,%d,%lf,%d", &grow_x, &grow_y, &grow_tol, &grow_label) < 3) { argc = 0; break; }
            grow = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    char morph_op[8] = "";
    int morph_radius = 0, morph_label = -1;
    bool morph = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--morph")) {
            if (std::sscanf(argv[i + 1], "%7[a-z],%d,%d", morph_op, &morph_radius, &morph_label) < 2) { argc = 0; break; }
            morph = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    char margin_op[8] = "";
    double margin_radius = 0.0;
    int margin_label = -1;
    bool margin = false;
    double smooth_radius = 0.0;
    int smooth_iterations = 1, smooth_label = -1;
    bool smooth = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--smooth")) {
            if (std::sscanf(argv[i + 1], "%lf,%d,%d", &smooth_radius, &smooth_iterations, &smooth_label) < 1) { argc = 0; break; }
            smooth = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--margin")) {
            if (std::sscanf(argv[i + 1], "%7[a-z],%lf,%d", margin_op, &margin_radius, &margin_label) < 2) { argc = 0; break; }
            margin = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    char islands_op[8] = "";
    long long islands_n = 0;
    int islands_label = -1;
    bool islands = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--islands")) {
            if (std::sscanf(argv[i + 1], "%7[a-z],%lld,%d", islands_op, &islands_n, &islands_label) < 2) { argc = 0; break; }
            islands = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; ++i) // the option and its value leave the positional arguments
        if (!std::strcmp(argv[i], "--light-color")) {
            if (std::sscanf(argv[i + 1], "%f,%f,%f", &key_color[0], &key_color[1], &key_color[2]) != 3) { argc = 0; break; }
            colored = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    std::vector<double> scissors_points;
    char scissors_op[16] = "";
    int scissors_label = -1;
    bool scissors = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--scissors")) {
            int used = 0;
            if (std::sscanf(argv[i + 1], "%15[a-z_],%d%n", scissors_op, &scissors_label, &used) < 2) { argc = 0; break; }
            for (const char* at = argv[i + 1] + used; *at == ',';) {
                char* end = nullptr;
                scissors_points.push_back(std::strtod(at + 1, &end));
                if (end == at + 1) { scissors_points.clear(); break; }
                at = end;
            }
            if (scissors_points.size() < 6 || (scissors_points.size() & 1)) { argc = 0; break; }
            scissors = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    struct CompeteBall { int label, x, y, z, r; };
    std::vector<CompeteBall> compete_balls;
    int compete_cost = 0, compete_shift = 0;
    long long compete_limit = 0;
    bool compete = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--compete")) {
            int used = 0;
            if (std::sscanf(argv[i + 1], "%d,%d,%lld%n", &compete_cost, &compete_shift, &compete_limit, &used) < 3) { argc = 0; break; }
            for (const char* at = argv[i + 1] + used; *at == ',';) {
                CompeteBall b{};
                int n = 0;
                if (std::sscanf(at + 1, "%d@%d,%d,%d,%d%n", &b.label, &b.x, &b.y, &b.z, &b.r, &n) < 5) { compete_balls.clear(); break; }
                compete_balls.push_back(b);
                at += 1 + n;
            }
            if (compete_balls.empty() || compete_limit < 0 || compete_limit > 0xFFFFFFll) { argc = 0; break; }
            compete = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    std::vector<int32_t> paint_points;
    int paint_label = -1;
    double paint_radius = 0.0;
    bool paint = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--paint")) {
            int used = 0;
            if (std::sscanf(argv[i + 1], "%d,%lf@%n", &paint_label, &paint_radius, &used) < 2 || used == 0) { argc = 0; break; }
            for (const char* at = argv[i + 1] + used;;) {
                double v[3];
                int n = 0;
                if (std::sscanf(at, "%lf,%lf,%lf%n", &v[0], &v[1], &v[2], &n) < 3) { paint_points.clear(); break; }
                for (double c : v) paint_points.push_back((int32_t) std::nearbyint(8.0 * c));
                at += n;
                if (*at != ';') {
                    if (*at) paint_points.clear();
                    break;
                }
                ++at;
            }
            if (paint_points.empty()) { argc = 0; break; }
            paint = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    int surface_label = -1;
    std::string surface_file;
    bool surface = false;
    for (int i = 1; i + 1 < argc; ++i)
        if (!std::strcmp(argv[i], "--surface")) {
            int used = 0;
            if (std::sscanf(argv[i + 1], "%d,%n", &surface_label, &used) < 1 || used == 0 || !argv[i + 1][used]) { argc = 0; break; }
            surface_file = argv[i + 1] + used;
            surface = true;
            for (int k = i; k + 2 < argc; ++k) argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s volume.mhd out.ppm [width height steps] [--light-color r,g,b] [--auto-window[=LOW,HIGH]] [--pick X,Y] [--grow X,Y,TOL[,LABEL]] [--morph OP,R[,LABEL]] [--margin OP,RADIUS[,LABEL]] [--smooth RADIUS[,ITERATIONS[,LABEL]]] [--islands OP,N[,LABEL]] [--scissors OP,LABEL,x0,y0,x1,y1,x2,y2[,..]] [--compete COST,SHIFT,LIMIT,LABEL@X,Y,Z,R[,LABEL@X,Y,Z,R..]] [--paint LABEL,RADIUS@X,Y,Z[;X,Y,Z..]] [--surface LABEL,FILE.obj]\n", argv[0]);
        return 2;
    }
    const int width = argc > 3 ? std::atoi(argv[3]) : 512, height = argc > 4 ? std::atoi(argv[4]) : 512;
    const float steps = argc > 5 ? (float) std::atof(argv[5]) : 256.0f;

    ARaymarchVolume volume;
    volume.bColoredLights = colored; // (read when the resources are initialised: before the volume is loaded)
    FVolumeInfo info;
    if (!LoadMHDFileIntoVolumeNormalized(volume, argv[1], &info)) { // RaymarchVolume.cpp:596-612
        std::fprintf(stderr, "could not load %s: %s\n", argv[1], tbrm_last_error());
        return 1;
    }
    std::printf("volume %d x %d x %d, values %g .. %g\n", info.Dimensions[0], info.Dimensions[1], info.Dimensions[2], info.MinValue, info.MaxValue);

    // window the upper half of the value range (window units are the file's units: FVolumeInfo::NormalizeValue / Range)
    volume.SetWindowCenter(info.NormalizeValue(info.MinValue + 0.6f * (info.MaxValue - info.MinValue)));
    volume.SetWindowWidth(info.NormalizeRange(0.8f * (info.MaxValue - info.MinValue)));
    if (auto_window) { // ... or the window the data proposes; before the lights are set up, so that the first Tick propagates them through it
        if (!volume.AutoWindow(auto_low, auto_high)) {
            std::fprintf(stderr, "auto window failed: %s\n", tbrm_last_error());
            return 1;
        }
        std::printf("auto window %g .. %g percentile: center %g, width %g\n", auto_low, auto_high,
                    volume.RaymarchResources.WindowingParameters.Center, volume.RaymarchResources.WindowingParameters.Width);
    }
    volume.SetRaymarchSteps(steps);

    ARaymarchLight key, fill;
    key.ForwardVector = FVector{1, 0.35, -0.5};
    key.LightIntensity = 0.7f;
    for (int c = 0; c < 3; ++c) key.LightColor[c] = key_color[c];
    fill.ForwardVector = FVector{-0.4, 1, -0.3};
    fill.LightIntensity = 0.3f;
    volume.LightsArray = {&key, &fill};
    volume.Tick(0.016f); // first tick: recompute requested -> ResetAllLights

    tbrm_camera cam{};
    cam.position = FVector{-145, -95, 80};
    const double fl = std::sqrt(145.0 * 145 + 95.0 * 95 + 80.0 * 80);
    cam.forward = FVector{145 / fl, 95 / fl, -80 / fl};
    const double rl = std::sqrt(cam.forward.x * cam.forward.x + cam.forward.y * cam.forward.y);
    cam.right = FVector{cam.forward.y / rl, -cam.forward.x / rl, 0};
    cam.up = FVector{cam.right.y * cam.forward.z - cam.right.z * cam.forward.y, cam.right.z * cam.forward.x - cam.right.x * cam.forward.z,
        cam.right.x * cam.forward.y - cam.right.y * cam.forward.x};
    cam.tan_half_fov_y = std::tan(25.0 * 3.14159265358979323846 / 180.0);
    cam.tan_half_fov_x = cam.tan_half_fov_y * width / height;
    cam.width = width;
    cam.height = height;

    if (grow) { // before the frame, so that the frame shows the grown label
        FGrowResult g;
        if (!volume.GrowRegionAt(cam, grow_x, grow_y, 0.5f, grow_tol, grow_label, 6, g)) {
            std::fprintf(stderr, "grow failed: %s\n", tbrm_last_error());
            return 1;
        }
        std::vector<tbrm_label_stat> stats;
        if (!g.bSeeded) std::printf("grow %d,%d miss\n", grow_x, grow_y);
        else if (!volume.GetLabelStatistics(stats)) {
            std::fprintf(stderr, "label statistics failed: %s\n", tbrm_last_error());
            return 1;
        } else {
            const tbrm_label_stat& s = stats[(size_t) (grow_label & 255)];
            std::printf("grow %d,%d seed %d %d %d range %.9g .. %.9g voxels %llu box %d %d %d .. %d %d %d label %d mean %.9g\n", grow_x, grow_y, g.Seed[0], g.Seed[1],
                        g.Seed[2], g.LoUsed, g.HiUsed, (unsigned long long) g.Voxels, g.BoxMin[0], g.BoxMin[1], g.BoxMin[2], g.BoxMax[0], g.BoxMax[1], g.BoxMax[2],
                        grow_label, s.count > s.nan_count ? s.sum / (double) (s.count - s.nan_count) : 0.0);
        }
    }
    if (morph) { // after the grow, before the frame
        static const char* const names[4] = {"dilate", "erode", "open", "close"};
        int op = -1;
        for (int k = 0; k < 4; ++k)
            if (!std::strcmp(morph_op, names[k])) op = k;
        if (morph_label < 0) morph_label = grow_label;
        FMorphResult m;
        if (!volume.MorphLabel(op, morph_radius, morph_label, m)) {
            std::fprintf(stderr, "morph failed: %s\n", op < 0 ? "OP must be dilate, erode, open or close" : tbrm_last_error());
            return 1;
        }
        std::printf("morph %s %d label %d source %llu result %llu added %llu removed %llu box %d %d %d .. %d %d %d launches %d\n", morph_op, morph_radius,
                    morph_label, (unsigned long long) m.SourceVoxels, (unsigned long long) m.ResultVoxels, (unsigned long long) m.Added,
                    (unsigned long long) m.Removed, m.BoxMin[0], m.BoxMin[1], m.BoxMin[2], m.BoxMax[0], m.BoxMax[1], m.BoxMax[2], m.Launches);
    }
    if (margin) { // after the grow and the morphology, before the frame
        static const char* const names[4] = {"expand", "shrink", "open", "close"};
        int op = -1;
        for (int k = 0; k < 4; ++k)
            if (!std::strcmp(margin_op, names[k])) op = k;
        if (margin_label < 0) margin_label = grow_label;
        FMarginResult m;
        if (op < 0 || !volume.MarginLabel(op, margin_radius, margin_label, m)) {
            std::fprintf(stderr, "margin failed: %s\n", op < 0 ? "OP must be expand, shrink, open or close" : tbrm_last_error());
            return 1;
        }
        std::printf("margin %s %.9g label %d weights %u %u %u limit %u reach %d %d %d source %llu result %llu added %llu removed %llu box %d %d %d .. %d %d %d launches %d\n",
                    margin_op, margin_radius, margin_label, m.Weights[0], m.Weights[1], m.Weights[2], m.Limit, m.Reach[0], m.Reach[1], m.Reach[2],
                    (unsigned long long) m.SourceVoxels, (unsigned long long) m.ResultVoxels, (unsigned long long) m.Added, (unsigned long long) m.Removed,
                    m.BoxMin[0], m.BoxMin[1], m.BoxMin[2], m.BoxMax[0], m.BoxMax[1], m.BoxMax[2], m.Launches);
    }
    if (smooth) { // after the grow, the morphology and the margin, before the frame
        if (smooth_label < 0) smooth_label = grow_label;
        FSmoothResult m;
        if (!volume.MedianLabel(smooth_label, smooth_radius, smooth_iterations, m)) {
            std::fprintf(stderr, "smooth failed: %s\n", tbrm_last_error());
            return 1;
        }
        std::printf("smooth %.9g iterations %d label %d radius %d %d %d reach %d %d %d source %llu result %llu added %llu removed %llu box %d %d %d .. %d %d %d launches %d\n",
                    smooth_radius, smooth_iterations, smooth_label, m.Radius[0], m.Radius[1], m.Radius[2], m.Reach[0], m.Reach[1], m.Reach[2],
                    (unsigned long long) m.SourceVoxels, (unsigned long long) m.ResultVoxels, (unsigned long long) m.Added, (unsigned long long) m.Removed,
                    m.BoxMin[0], m.BoxMin[1], m.BoxMin[2], m.BoxMax[0], m.BoxMax[1], m.BoxMax[2], m.Launches);
    }
    if (islands) { // after the grow, the morphology, the margin and the smoothing, before the frame
        if (islands_label < 0) islands_label = grow_label;
        FIslandsResult r;
        bool known = true, ok = false;
        if (islands_n < 0 || islands_n > 0x7fffffff) known = false;
        else if (!std::strcmp(islands_op, "keep")) ok = volume.KeepLargestIslands(islands_label, (int) islands_n, r);
        else if (!std::strcmp(islands_op, "remove")) ok = volume.RemoveSmallIslands(islands_label, (uint64_t) islands_n, r);
        else if (!std::strcmp(islands_op, "split")) ok = volume.SplitIslands(islands_label, islands_label, (int) islands_n, r);
        else if (!std::strcmp(islands_op, "fill")) ok = volume.FillLabelHoles(islands_label, r, islands_n == 0 ? UINT64_MAX : (uint64_t) islands_n);
        else known = false;
        if (!ok) {
            std::fprintf(stderr, "islands failed: %s\n", known ? tbrm_last_error() : "OP must be keep, remove, split or fill, N >= 0");
            return 1;
        }
        std::printf("islands %s %lld label %d set %llu islands %llu spared %llu kept %llu dropped %llu kept_voxels %llu dropped_voxels %llu largest %llu relabelled %llu box %d %d %d .. %d %d %d\n",
                    islands_op, islands_n, islands_label, (unsigned long long) r.SetVoxels, (unsigned long long) r.Islands, (unsigned long long) r.Spared,
                    (unsigned long long) r.Kept, (unsigned long long) r.Dropped, (unsigned long long) r.KeptVoxels, (unsigned long long) r.DroppedVoxels,
                    (unsigned long long) r.Largest, (unsigned long long) r.Relabelled, r.BoxMin[0], r.BoxMin[1], r.BoxMin[2], r.BoxMax[0], r.BoxMax[1], r.BoxMax[2]);
    }
    std::vector<float> rgba((size_t) width * height * 4);
    if (scissors) { // after every other edit, before the frame: the points are pixels of the frame below
        static const char* const names[4] = {"erase_inside", "erase_outside", "fill_inside", "fill_outside"};
        int op = -1;
        for (int k = 0; k < 4; ++k)
            if (!std::strcmp(scissors_op, names[k])) op = k;
        FScissorsResult m;
        if (op < 0 || !volume.ScissorLabel(cam, scissors_points, op, scissors_label, 0.0, HUGE_VAL, m)) {
            std::fprintf(stderr, "scissors failed: %s\n", op < 0 ? "OP must be erase_inside, erase_outside, fill_inside or fill_outside" : tbrm_last_error());
            return 1;
        }
        std::printf("scissors %s label %d points %zu pixels %llu source %llu result %llu added %llu removed %llu box %d %d %d .. %d %d %d bricks %d inside %d outside %d projected launches %d\n",
                    scissors_op, scissors_label, scissors_points.size() / 2, (unsigned long long) m.MaskPixels, (unsigned long long) m.SourceVoxels,
                    (unsigned long long) m.ResultVoxels, (unsigned long long) m.Added, (unsigned long long) m.Removed, m.BoxMin[0], m.BoxMin[1], m.BoxMin[2], m.BoxMax[0],
                    m.BoxMax[1], m.BoxMax[2], m.BricksInside, m.BricksOutside, m.BricksProjected, m.Launches);
    }
    if (compete) { // after every other edit, before the frame: the balls are painted over what is there, then everything else is competed for
        const int nx = info.Dimensions[0], ny = info.Dimensions[1], nz = info.Dimensions[2];
        std::vector<uint8_t> labels((size_t) nx * ny * nz, 0);
        std::vector<int> seeds;
        bool ok = tbrm_attach_empty_label_volume(volume.RaymarchResources.Handle) == TBRM_OK &&
                  tbrm_download_label_volume(volume.RaymarchResources.Handle, labels.data(), labels.size()) == TBRM_OK;
        for (const auto& b : compete_balls) {
            if (b.label < 1 || b.label > 255 || b.r < 0) { ok = false; break; }
            seeds.push_back(b.label);
            for (int z = std::max(b.z - b.r, 0); z <= std::min(b.z + b.r, nz - 1); ++z)
                for (int y = std::max(b.y - b.r, 0); y <= std::min(b.y + b.r, ny - 1); ++y)
                    for (int x = std::max(b.x - b.r, 0); x <= std::min(b.x + b.r, nx - 1); ++x)
                        if ((x - b.x) * (x - b.x) + (y - b.y) * (y - b.y) + (z - b.z) * (z - b.z) <= b.r * b.r) labels[((size_t) z * ny + y) * nx + x] = (uint8_t) b.label;
        }
        FCompeteOptions opt;
        opt.SpacingCost = compete_cost;
        opt.ValueShift = compete_shift;
        opt.CostLimit = (uint32_t) compete_limit;
        FCompeteResult m;
        if (!ok || !volume.SetLabelVolume(labels.data(), labels.size()) || !volume.GrowFromSeeds(seeds, opt, m)) {
            std::fprintf(stderr, "compete failed: %s\n", ok ? tbrm_last_error() : "LABEL must be 1 .. 255, R >= 0, and the volume must take labels");
            return 1;
        }
        std::printf("compete step %d %d %d shift %d limit %lld seeds %llu claimable %llu claimed %llu relabelled %llu max_cost %u box %d %d %d .. %d %d %d passes %d per_label",
                    m.StepCost[0], m.StepCost[1], m.StepCost[2], compete_shift, compete_limit, (unsigned long long) m.SeedVoxels, (unsigned long long) m.Claimable,
                    (unsigned long long) m.Claimed, (unsigned long long) m.Relabelled, m.MaxCost, m.BoxMin[0], m.BoxMin[1], m.BoxMin[2], m.BoxMax[0], m.BoxMax[1], m.BoxMax[2], m.Passes);
        for (int l = 0; l < 256; ++l)
            if (m.ClaimedPerLabel[l]) std::printf(" %d:%llu", l, (unsigned long long) m.ClaimedPerLabel[l]);
        std::printf("\n");
    }
    if (paint) { // after every other edit, before the frame
        FPaintResult m;
        if (tbrm_attach_empty_label_volume(volume.RaymarchResources.Handle) != TBRM_OK || !volume.PaintLabel(paint_points, paint_radius, paint_label, m)) {
            std::fprintf(stderr, "paint failed: %s\n", paint_label < 0 || paint_label > 255 ? "LABEL must be 0 .. 255" : tbrm_last_error());
            return 1;
        }
        std::printf("paint label %d radius %g points %d segments %d stamp %llu added %llu removed %llu relabelled %llu box %d %d %d .. %d %d %d bricks %d whole %d untouched %d evaluated launches %d\n",
                    paint_label, paint_radius, m.Points, m.Segments, (unsigned long long) m.StampVoxels, (unsigned long long) m.Added, (unsigned long long) m.Removed,
                    (unsigned long long) m.Relabelled, m.BoxMin[0], m.BoxMin[1], m.BoxMin[2], m.BoxMax[0], m.BoxMax[1], m.BoxMax[2], m.BricksWhole, m.BricksUntouched,
                    m.BricksEvaluated, m.Launches);
    }
    if (surface) { // after every edit, before the frame
        FLabelSurface m;
        if (!volume.ExtractLabelSurface(surface_label, m)) {
            std::fprintf(stderr, "surface failed: %s\n", surface_label < 0 || surface_label > 255 ? "LABEL must be 0 .. 255" : tbrm_last_error());
            return 1;
        }
        FILE* f = std::fopen(surface_file.c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "surface failed: cannot write %s\n", surface_file.c_str());
            return 1;
        }
        // the unit cube back to the file's units: voxel i at i * spacing
        const bool unit = volume.VoxelSpacing[0] == 0.0 && volume.VoxelSpacing[1] == 0.0 && volume.VoxelSpacing[2] == 0.0;
        const int size[3] = {volume.RaymarchResources.SizeX, volume.RaymarchResources.SizeY, volume.RaymarchResources.SizeZ};
        std::fprintf(f, "# label %d: %llu voxels, %llu vertices, %llu triangles\n", surface_label, (unsigned long long) m.SetVoxels, (unsigned long long) m.Vertices,
                     (unsigned long long) (2 * m.Quads));
        for (size_t i = 0; i < m.Positions.size(); i += 3) {
            double p[3];
            for (int c = 0; c < 3; ++c) p[c] = (double) m.Positions[i + c] * (size[c] - 1) * (unit ? 1.0 : volume.VoxelSpacing[c]);
            std::fprintf(f, "v %.6f %.6f %.6f\n", p[0], p[1], p[2]);
        }
        for (size_t i = 0; i < m.Normals.size(); i += 3) std::fprintf(f, "vn %.6f %.6f %.6f\n", m.Normals[i], m.Normals[i + 1], m.Normals[i + 2]);
        for (size_t i = 0; i < m.Triangles.size(); i += 3)
            std::fprintf(f, "f %u//%u %u//%u %u//%u\n", m.Triangles[i] + 1, m.Triangles[i] + 1, m.Triangles[i + 1] + 1, m.Triangles[i + 1] + 1, m.Triangles[i + 2] + 1, m.Triangles[i + 2] + 1);
        std::fclose(f);
        std::printf("surface label %d voxels %llu vertices %llu quads %llu axis %llu %llu %llu cells %d %d %d .. %d %d %d blocks %d evaluated %d skipped launches %d file %s\n", surface_label,
                    (unsigned long long) m.SetVoxels, (unsigned long long) m.Vertices, (unsigned long long) m.Quads, (unsigned long long) m.QuadsAxis[0], (unsigned long long) m.QuadsAxis[1],
                    (unsigned long long) m.QuadsAxis[2], m.CellMin[0], m.CellMin[1], m.CellMin[2], m.CellMax[0], m.CellMax[1], m.CellMax[2], m.BlocksEvaluated, m.BlocksSkipped, m.Launches,
                    surface_file.c_str());
    }
    if (!volume.RenderLit(cam, rgba.data())) {
        std::fprintf(stderr, "render failed: %s\n", tbrm_last_error());
        return 1;
    }
    double coverage = 0;
    std::vector<unsigned char> rgb((size_t) width * height * 3);
    for (size_t i = 0; i < (size_t) width * height; ++i) {
        coverage += rgba[4 * i + 3];
        for (int c = 0; c < 3; ++c) // premultiplied colour over black, display gamma 2.2
            rgb[3 * i + c] = (unsigned char) std::lround(255.0 * std::pow(std::min(std::max((double) rgba[4 * i + c], 0.0), 1.0), 1.0 / 2.2));
    }
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 1;
    std::fprintf(f, "P6\n%d %d\n255\n", width, height);
    std::fwrite(rgb.data(), 1, rgb.size(), f);
    std::fclose(f);
    std::printf("wrote %s (%d x %d, mean alpha %.4f)\n", argv[2], width, height, coverage / ((double) width * height));
    if (pick) {
        FVolumeHit hit;
        if (!volume.PickVolume(cam, pick_x, pick_y, 0.5f, hit)) {
            std::fprintf(stderr, "pick failed: %s\n", tbrm_last_error());
            return 1;
        }
        if (hit.bHit) std::printf("pick %d,%d hit sample %d world %.9g %.9g %.9g depth %.9g value %.9g label %d\n", pick_x, pick_y, hit.Sample,
                                  hit.WorldPosition.x, hit.WorldPosition.y, hit.WorldPosition.z, hit.Depth, (double) hit.Value, hit.Label);
        else std::printf("pick %d,%d miss\n", pick_x, pick_y);
    }
    return 0;
}
