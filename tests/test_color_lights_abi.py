"""The C-ABI of coloured directional lights (include/tbrm_color_lights.h): exported and bound, null handles refused, the struct's
layout, the C++ facade's colour members (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from tbraymarcherplugin_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tbrm_color_lights.h")


def declared_symbols():
    return re.findall(r"TBRM_API\s+[\w\s\*]+?\b(tbrm_\w+)\s*\(", open(HEADER).read())


def test_header_symbols_are_exported_and_bound():
    lib = abi.load()
    declared = declared_symbols()
    assert sorted(declared) == sorted(abi.COLOR_LIGHT_SYMBOLS), set(declared) ^ set(abi.COLOR_LIGHT_SYMBOLS)
    assert not set(declared) & set(abi.SYMBOLS)
    assert not set(declared) & set(abi.LABEL_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in tbrm_color_lights.h but not exported by libtbrm.so"
    version = int(re.search(r"#define\s+TBRM_COLOR_LIGHTS_ABI_VERSION\s+(\d+)", open(HEADER).read()).group(1))
    assert lib.tbrm_color_lights_abi_version() == version == abi.COLOR_LIGHTS_ABI_VERSION == 1


def test_every_handle_taking_entry_point_rejects_a_null_handle():
    lib = abi.load()
    z = C.c_void_p(None)
    buf = (C.c_float * 16)()
    light = abi.ColorDirLight((1.0, 0.2, -0.3), 0.5, (1.0, 0.5, 0.0))
    world = abi.make_world()
    flag = C.c_int(7)
    calls = {
        "tbrm_add_color_dir_light": lambda: lib.tbrm_add_color_dir_light(z, C.byref(light), 1, C.byref(world), C.byref(flag)),
        "tbrm_change_color_dir_light": lambda: lib.tbrm_change_color_dir_light(z, C.byref(light), C.byref(light), C.byref(world), C.byref(flag)),
        "tbrm_download_light_channel": lambda: lib.tbrm_download_light_channel(z, 0, buf, 4),
        "tbrm_upload_light_channel": lambda: lib.tbrm_upload_light_channel(z, 0, buf, 4),
    }
    for name, call in calls.items():
        abi.set_tunable("ray_labels", 0)   # (clears nothing: the message checked below is this call's own)
        assert call() == abi.ERR_INVALID_ARG, name
        assert b"null" in lib.tbrm_last_error(), name
    assert flag.value == 0   # a refused operator reports that no light was added
    abi.set_tunable("ray_labels", 0)
    assert lib.tbrm_resources_light_channels(z) == 0 and b"null" in lib.tbrm_last_error()
    out = C.c_void_p(1)
    assert lib.tbrm_resources_create_rgb(None, C.byref(out)) == abi.ERR_INVALID_ARG and lib.tbrm_last_error()
    free = {"tbrm_color_lights_abi_version", "tbrm_resources_create_rgb", "tbrm_resources_light_channels"}
    assert set(abi.COLOR_LIGHT_SYMBOLS) == set(calls) | free


def test_color_dir_light_layout_matches_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "tbrm_color_lights.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu\\n", sizeof(tbrm_color_dir_light), offsetof(tbrm_color_dir_light, light),\n'
                   "         offsetof(tbrm_color_dir_light, color), sizeof(tbrm_dir_light_params));\n"
                   "  return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    size, off_light, off_color, size_light = (int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(abi.ColorDirLight) == size
    assert abi.ColorDirLight.light.offset == off_light == 0
    assert abi.ColorDirLight.color.offset == off_color == size_light == C.sizeof(abi.DirLightParams)
    l = abi.ColorDirLight((1.0, 2.0, 3.0), 0.25, (0.1, 0.2, 0.3))
    assert (l.light.light_direction.z, l.light.light_intensity) == (3.0, 0.25)
    assert list(l.color) == [C.c_float(v).value for v in (0.1, 0.2, 0.3)]
    assert list(abi.ColorDirLight((1.0, 0.0, 0.0), 1.0).color) == [1.0, 1.0, 1.0]   # white unless told otherwise


def test_facade_color_members_compile_with_gxx(tmp_path, abi_mod):
    src = tmp_path / "color_facade.cpp"
    src.write_text('#include "tbrm_plugin.hpp"\n#include "tbrm_color_lights.h"\n#include <cstdio>\n'
                   "int main() {\n"
                   "  tbrm_plugin::ARaymarchVolume v;\n"
                   "  tbrm_plugin::ARaymarchLight l;\n"
                   "  const bool white = l.LightColor[0] == 1.0f && l.LightColor[1] == 1.0f && l.LightColor[2] == 1.0f && !v.bColoredLights;\n"
                   "  v.bColoredLights = true;\n"
                   "  l.LightColor[1] = 0.5f;\n"
                   "  const tbrm_color_dir_light c = l.GetCurrentColorParameters();\n"
                   "  tbrm_world_params w{};\n"
                   "  int added = 1;\n"
                   "  const int e1 = tbrm_add_color_dir_light(v.RaymarchResources.Handle, &c, 1, &w, &added);\n"
                   "  const int e2 = tbrm_change_color_dir_light(v.RaymarchResources.Handle, &c, &c, &w, &added);\n"
                   "  const bool refused = e1 == TBRM_ERR_INVALID_ARG && e2 == TBRM_ERR_INVALID_ARG && added == 0 && tbrm_resources_light_channels(v.RaymarchResources.Handle) == 0;\n"
                   '  std::printf("%s %s %d\\n", white ? "white" : "tinted", refused ? "refused" : "accepted", (int) (c.color[1] == 0.5f));\n'
                   "  return 0; }\n")
    exe = str(tmp_path / "color_facade")
    lib_dir = os.path.join(ROOT, "tbraymarcherplugin_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", lib_dir, "-ltbrm", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "white refused 1"   # a volume without a handle refuses the colour calls
