// Renderer.hpp — host-side mirror of the reference's draw-call interface, over the C-ABI.
//
// The reference's host language is Swift (renderer/Renderer.swift, renderer/GpuRenderer.swift);
// this image has no Swift toolchain, so the host side above include/swr.h is written in C++ with
// the SAME type and method names, argument meaning and defaults, so that call sites read like
// the reference's (App.swift:153-185):
//
//     RenderPass pass{image, depthImage, vertices, indices};   // Renderer.swift:191-200
//     pass.primitiveType = PrimitiveType::triangle;            // App.swift:164
//     pass.transform = projectionMatrix * transform.matrix;    // App.swift:183
//     renderer.render(pass);                                   // App.swift:185
//
// The Swift façade a maintainer would drop into the app is in host/swift/ (see INTEGRATION.md).
//
// Error behaviour: the reference has no error channel — it traps (fatalError / assert / try!,
// Renderer.swift:26,209,239; GpuRenderer.swift:20-38).  The closest C++ analogue is an exception:
// every non-zero swr status is thrown as swr_host::RenderError carrying swr_last_error().
// There is no CPU fallback: constructing a renderer without a HIP device throws.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/swr.h"

namespace swr_host {

struct RenderError : std::runtime_error {
    int code;
    RenderError(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

// Renderer.swift:44-49 — memory order b,g,r,a.
struct Pixel {
    uint8_t b, g, r, a;
};
static_assert(sizeof(Pixel) == 4, "Pixel is BGRA8");

// Renderer.swift:8-42 — a non-owning view of caller memory; element (x,y) at pointer[y*width+x]
// (App.swift:351-360: bytesPerRow is stored but addressing uses width).
template <class P>
class Image {
public:
    Image(P* pointer, long width, long height, long bytesPerRow)
        : pointer(pointer), width(width), height(height), bytesPerRow(bytesPerRow) {}
    P* pointer;
    const long width, height, bytesPerRow;
    bool contains(long x, long y) const { return x >= 0 && x < width && y >= 0 && y < height; }
    // get: the reference fatalError()s out of bounds (Renderer.swift:24-29)
    const P& at(long x, long y) const {
        if (!contains(x, y)) throw RenderError(SWR_ERR_BAD_ARG, "Image subscript out of bounds");
        return pointer[y * width + x];
    }
    // set: silently dropped out of bounds (Renderer.swift:30-36)
    void set(long x, long y, const P& v) {
        if (contains(x, y)) pointer[y * width + x] = v;
    }
};
using ColorImage = Image<Pixel>;   // Renderer.swift:5
using DepthImage = Image<float>;   // Renderer.swift:6

// Renderer.swift:154-157 — two SIMD3<Float>, 16 bytes each (lane 3 is padding).
struct Vertex {
    float xyz[4];
    float color[4];
    Vertex() : xyz{0, 0, 0, 0}, color{0, 0, 0, 0} {}
    Vertex(float x, float y, float z, float r, float g, float b) : xyz{x, y, z, 0}, color{r, g, b, 0} {}
};
static_assert(sizeof(Vertex) == sizeof(swr_vertex), "Vertex must match swr_vertex");

// Renderer.swift:174-189
enum class PrimitiveType { triangle, line, vertices };
inline int verticesCount(PrimitiveType t) { return t == PrimitiveType::line ? 2 : 3; }

// matrix_float4x4: column-major, columns[c][r] (Renderer.swift:199; default = identity).
struct matrix_float4x4 {
    float columns[4][4];
    static matrix_float4x4 identity() {
        matrix_float4x4 m{};
        for (int i = 0; i < 4; i++) m.columns[i][i] = 1.0f;
        return m;
    }
    // matrix_float4x4(rows:) as used at App.swift:176-181
    static matrix_float4x4 fromRows(const float r[4][4]) {
        matrix_float4x4 m{};
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) m.columns[j][i] = r[i][j];
        return m;
    }
    friend matrix_float4x4 operator*(const matrix_float4x4& a, const matrix_float4x4& b) {
        matrix_float4x4 o{};
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++) {
                float s = 0.0f;
                for (int k = 0; k < 4; k++) s += a.columns[k][r] * b.columns[c][k];
                o.columns[c][r] = s;
            }
        return o;
    }
};

// ---- fragment-stage extensions (not in the reference; include/swr.h swr_vertex_attr / swr_material) ----
// Per-vertex normal + texture coordinate, parallel to RenderPass.vertices.
struct VertexAttributes {
    float normal[4];
    float uv[4];
    VertexAttributes() : normal{0, 0, 0, 0}, uv{0, 0, 0, 0} {}
    VertexAttributes(float nx, float ny, float nz, float u, float v) : normal{nx, ny, nz, 0}, uv{u, v, 0, 0} {}
};
static_assert(sizeof(VertexAttributes) == sizeof(swr_vertex_attr), "VertexAttributes must match swr_vertex_attr");

enum class Shader { passthrough = SWR_SHADER_PASSTHROUGH, phong = SWR_SHADER_PHONG,
                    texturedPhong = SWR_SHADER_TEXTURED_PHONG };

// What the Metal pipeline would bind as fragment-function arguments.
struct Material {
    Shader shader = Shader::passthrough;       // passthrough = Shaders.metal:116-121
    int shininessLog2 = 5;                     // specular exponent 2^k
    float lightDirection[3] = {0, 0, -1};      // unit, towards the light, in the space of the normals
    float halfDirection[3] = {0, 0, -1};       // unit Blinn half vector
    float ambient = 0.15f, diffuse = 0.8f, specular = 0.4f;
    const Image<Pixel>* texture = nullptr;     // texturedPhong only; caller-owned b,g,r,a texels
};

// A render pass's load action (Metal's MTLLoadAction; include/swr.h SWR_FLAG_LOAD): clear = the reference's render(renderPass:)
// (Renderer.swift:205-206 clear first); load = the pass draws on top of what colorBuffer / depthBuffer already hold.
enum class LoadAction { clear, load };

// Face culling (Metal's MTLCullMode / MTLWinding; include/swr.h "Face culling"): which facing is not drawn, and which winding as
// displayed is the front.  The defaults draw every triangle, as the reference does.
enum class CullMode { none, front, back };
enum class Winding { clockwise, counterClockwise };
inline uint32_t faceCullingFlags(CullMode cullMode, Winding frontFacingWinding) {
    return (cullMode == CullMode::back ? (uint32_t)SWR_FLAG_CULL_BACK : 0u) |
           (cullMode == CullMode::front ? (uint32_t)SWR_FLAG_CULL_FRONT : 0u) |
           (frontFacingWinding == Winding::counterClockwise ? (uint32_t)SWR_FLAG_FRONT_CCW : 0u);
}

// Depth clipping (Metal's MTLDepthClipMode; include/swr.h "Depth clipping"): none = the reference (every vertex straight to xyz / w);
// clip = triangles clipped against the near (z >= 0) and far (z <= w) planes before the divide.
enum class DepthClipMode { none, clip };
inline uint32_t depthClipFlags(DepthClipMode mode) { return mode == DepthClipMode::clip ? (uint32_t)SWR_FLAG_DEPTH_CLIP : 0u; }

// How colour and the varyings are interpolated (include/swr.h "Perspective-correct interpolation"): screenLinear = the reference
// (the screen-space weights); perspective = corrected by the clip-space w of each corner, like Metal's [[center_perspective]].
enum class InterpolationMode { screenLinear, perspective };
inline uint32_t interpolationFlags(InterpolationMode mode) {
    return mode == InterpolationMode::perspective ? (uint32_t)SWR_FLAG_PERSPECTIVE : 0u;
}

// Alpha blending (include/swr.h "Alpha blending"; Metal's isBlendingEnabled on the colour attachment): a renderer whose blend state is
// enabled draws every triangle pass as a blend frame — every fragment blended into the image in draw order, the depth image never
// written.  opacity 0..255; the passthrough material only.
enum class BlendMode : int32_t { over = SWR_BLEND_OVER, add = SWR_BLEND_ADD };
struct BlendState {
    bool enabled = false;
    BlendMode mode = BlendMode::over;
    int32_t opacity = 255;
};

// Renderer.swift:191-200 (+ the optional extended fragment stage: empty attributes / passthrough material
// = the reference's RenderPass exactly; + the load action, clear by default = the reference; + face culling, none by default;
// + depth clipping, none by default; + the interpolation mode, screen-linear by default)
struct RenderPass {
    ColorImage colorBuffer;
    DepthImage depthBuffer;
    std::vector<Vertex> vertices;
    std::vector<int64_t> indices;                       // Swift Int
    PrimitiveType primitiveType = PrimitiveType::triangle;
    matrix_float4x4 transform = matrix_float4x4::identity();
    std::vector<VertexAttributes> attributes = {};
    Material material = {};
    LoadAction loadAction = LoadAction::clear;
    CullMode cullMode = CullMode::none;
    Winding frontFacingWinding = Winding::clockwise;
    DepthClipMode depthClipMode = DepthClipMode::none;
    InterpolationMode interpolationMode = InterpolationMode::screenLinear;
};

// One draw of a draw list (swr_draw_item, include/swr.h): indices [firstIndex, firstIndex + indexCount) of the resident scene
// drawn with their own transform — several meshes or draw calls of one render pass, or instances of one mesh, in one frame.
struct DrawItem {
    int64_t firstIndex = 0;             // multiple of 3
    int64_t indexCount = 0;             // multiple of 3
    matrix_float4x4 transform = matrix_float4x4::identity();
};

namespace detail {
class Context {
public:
    // deviceCount > 1: one context drives that many tile-row bands, on as many GPUs as are visible (swr_config.device_count)
    explicit Context(uint32_t deviceCount = 0) {
        swr_config cfg{deviceCount > 1 ? 0 : -1, deviceCount, 0, 0};
        int rc = swr_context_create(&cfg, &ctx_);
        if (rc) throw RenderError(rc, swr_last_error(nullptr));
    }
    ~Context() { swr_context_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    // sceneId != 0: the caller's promise that p.vertices / p.indices / p.attributes / the texture hold what they held at
    // the last call with this id (swr_render_pass.scene_id): nothing is uploaded, the pass costs one resident frame + the gather
    void render(const RenderPass& p, uint32_t flags, uint64_t sceneId = 0, const BlendState& blend = BlendState{}) {
        if (blend.enabled) {
            const swr_blend b{(int32_t)blend.mode, blend.opacity, {0, 0}};
            const int rcb = swr_blend_set(ctx_, &b);
            if (rcb) throw RenderError(rcb, swr_last_error(ctx_));
            flags |= (uint32_t)SWR_FLAG_BLEND;
        }
        swr_render_pass rp{};
        rp.scene_id = sceneId;
        rp.color = p.colorBuffer.pointer;
        rp.depth = p.depthBuffer.pointer;
        rp.width = p.colorBuffer.width;
        rp.height = p.colorBuffer.height;
        rp.color_bytes_per_row = p.colorBuffer.bytesPerRow;
        rp.depth_bytes_per_row = p.depthBuffer.bytesPerRow;
        rp.vertices = reinterpret_cast<const swr_vertex*>(p.vertices.data());
        rp.vertex_count = (int64_t)p.vertices.size();
        rp.indices = p.indices.data();
        rp.index_count = (int64_t)p.indices.size();
        rp.primitive_type = (int32_t)p.primitiveType;
        rp.flags = flags | (p.loadAction == LoadAction::load ? (uint32_t)SWR_FLAG_LOAD : 0u) |
                   faceCullingFlags(p.cullMode, p.frontFacingWinding) | depthClipFlags(p.depthClipMode) |
                   interpolationFlags(p.interpolationMode);
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++) rp.transform[4 * c + r] = p.transform.columns[c][r];
        swr_material mat{};
        if (p.material.shader != Shader::passthrough) {
            if (p.attributes.size() != p.vertices.size())
                throw RenderError(SWR_ERR_BAD_ARG, "RenderPass.attributes must have one entry per vertex");
            mat.shader = (int32_t)p.material.shader;
            mat.shininess_log2 = p.material.shininessLog2;
            for (int k = 0; k < 3; k++) {
                mat.light_dir[k] = p.material.lightDirection[k];
                mat.half_dir[k] = p.material.halfDirection[k];
            }
            mat.ambient = p.material.ambient; mat.diffuse = p.material.diffuse; mat.specular = p.material.specular;
            rp.attributes = reinterpret_cast<const swr_vertex_attr*>(p.attributes.data());
            rp.material = &mat;
            if (p.material.shader == Shader::texturedPhong) {
                if (!p.material.texture) throw RenderError(SWR_ERR_BAD_ARG, "texturedPhong needs Material.texture");
                rp.texture = p.material.texture->pointer;
                rp.tex_width = (int32_t)p.material.texture->width;
                rp.tex_height = (int32_t)p.material.texture->height;
            }
        }
        int rc = swr_render(ctx_, &rp);
        if (rc) throw RenderError(rc, swr_last_error(ctx_));
    }
    // One frame of several draws (swr_draw_list) on the scene and target the last render() with a sceneId left resident; the
    // image is the context's, as after that render() (its colour / depth buffers are not written).  The cull mode and winding hold
    // for every item; each item's facing comes from its own transform.
    void drawList(const std::vector<DrawItem>& items, uint32_t flags, CullMode cullMode = CullMode::none,
                  Winding frontFacingWinding = Winding::clockwise, DepthClipMode depthClipMode = DepthClipMode::none,
                  InterpolationMode interpolationMode = InterpolationMode::screenLinear) {
        std::vector<swr_draw_item> list(items.size());
        for (size_t k = 0; k < items.size(); k++) {
            list[k].first_index = items[k].firstIndex;
            list[k].index_count = items[k].indexCount;
            for (int c = 0; c < 4; c++)
                for (int r = 0; r < 4; r++) list[k].transform[4 * c + r] = items[k].transform.columns[c][r];
        }
        int rc = swr_draw_list(ctx_, list.data(), (int32_t)list.size(), flags | faceCullingFlags(cullMode, frontFacingWinding) |
                                                                      depthClipFlags(depthClipMode) |
                                                                      interpolationFlags(interpolationMode));
        if (rc) throw RenderError(rc, swr_last_error(ctx_));
    }
    // The ID image of the last frame, drawn with SWR_FLAG_PRIMITIVE_IDS (swr_read_ids): width * height words, the triangle index (draw
    // lists: the position in the concatenation of the items) visible at every pixel, SWR_ID_NONE where the frame kept no fragment.
    void readPrimitiveIds(uint32_t* dst) {
        int rc = swr_read_ids(ctx_, dst);
        if (rc) throw RenderError(rc, swr_last_error(ctx_));
    }
private:
    swr_context* ctx_ = nullptr;
};
}  // namespace detail

// final class Renderer { func render(renderPass:) } (Renderer.swift:202-230): the CPU renderer's
// semantics exactly as written — painter's order, depth image left at +inf — executed on the GPU.
class Renderer {
public:
    // The reference's caller draws the same mesh every display frame with a new transform (App.swift:153-185).
    // staticScene = true tells the renderer so: the mesh of the first render(renderPass:) stays resident on the GPU
    // (what GpuRenderer.swift:32-33,41-67 does with its MTLBuffers) until sceneVersion is changed or the vertex / index
    // counts differ.  false (the default) uploads on every call, whatever the arrays hold.
    bool staticScene = false;
    uint64_t sceneVersion = 1;          // bump after editing the arrays of a static scene in place
    // .line passes: false (default) = the reference as written — draw(line:colorBuffer:depthBuffer:) is an empty stub
    // (Renderer.swift:289-293), the pass only clears; true = draw every line with the reference's own DDA
    // (draw(line:with:in:), Renderer.swift:405-419; SWR_FLAG_REAL_LINES)
    bool realLines = false;
    BlendState blend;                   // enabled: triangle passes are blend frames (SWR_FLAG_BLEND), usually with LoadAction::load
    void render(const RenderPass& renderPass) {
        const bool lines = realLines && renderPass.primitiveType == PrimitiveType::line;
        ctx_.render(renderPass, lines ? (uint32_t)SWR_FLAG_REAL_LINES : 0u, staticScene ? sceneVersion : 0, blend);
    }
private:
    detail::Context ctx_;
};

// final class GpuRenderer { func render(renderPass:) } (GpuRenderer.swift:12,35): same pixel rules
// as Renderer (the parity target), with the z-test the Metal path has (Shaders.metal:158-165)
// restored from Renderer.swift:257-261.  depthTest = false gives Renderer's output.
class GpuRenderer {
public:
    GpuRenderer() = default;
    // One renderer, N GPUs: the framebuffer is cut into N tile-row bands and every band is copied straight into its rows
    // of RenderPass.colorBuffer / .depthBuffer (the reference has exactly one synchronous draw call, GpuRenderer.swift:35).
    explicit GpuRenderer(uint32_t deviceCount) : ctx_(deviceCount) {}
    bool depthTest = true;
    // true: the Metal kernels' own rules (round() snap, ROI threads + inside test, UNORM rounding,
    // ROI-min == 0 skip; Shaders.metal:57-167, GpuRenderer.swift:122-124) instead of the CPU renderer's
    bool metalRules = false;
    // see Renderer::staticScene: the resident mesh of GpuRenderer.swift:32-33,41-67
    bool staticScene = false;
    uint64_t sceneVersion = 1;
    bool realLines = false;             // see Renderer::realLines
    // true: every render() also writes the ID image (SWR_FLAG_PRIMITIVE_IDS; triangle passes only), read with readPrimitiveIds —
    // what a Metal app gets from a second colour attachment written with [[primitive_id]]
    bool primitiveIds = false;
    BlendState blend;                   // see Renderer::blend (not together with primitiveIds: SWR_ERR_UNSUPPORTED)
    void render(const RenderPass& renderPass) {
        const bool lines = realLines && renderPass.primitiveType == PrimitiveType::line;
        ctx_.render(renderPass, (metalRules ? (uint32_t)SWR_FLAG_METAL_RULES : (depthTest ? (uint32_t)SWR_FLAG_DEPTH_TEST : 0u)) |
                                    (lines ? (uint32_t)SWR_FLAG_REAL_LINES : 0u) | (primitiveIds ? (uint32_t)SWR_FLAG_PRIMITIVE_IDS : 0u),
                    staticScene ? sceneVersion : 0, blend);
    }
    // the ID image of the last render() (primitiveIds = true): colorBuffer.width * height words, row-major (mouse picking)
    void readPrimitiveIds(uint32_t* dst) { ctx_.readPrimitiveIds(dst); }
private:
    detail::Context ctx_;
};

}  // namespace swr_host
