// urt_types.h — byte layouts the C-ABI accepts.  They are the reference's own structured-buffer
// layouts (C# sequential structs, 4-byte fields, no padding):
//   RayTraceParams  40 B   Assets/Scripts/RayTraceMaster.cs:48-53  / RayTraceShader.compute:29-34
//   MeshObject     112 B   RayTraceMaster.cs:82-86                 / RayTraceShader.compute:43-49
//   Sphere          56 B   RayTraceMaster.cs:116-119               / RayTraceShader.compute:51-55
//   BVHNode         28 B   RayTraceMaster.cs:148-152               / RayTraceShader.compute:57-61
// Strides are asserted by the reference at RayTraceMaster.cs:42-45 and used at :738-745.
// The ray-query records (urt_ray_query, urt.h) are the library's own: 16-byte aligned rows for coalesced dwordx4 loads and stores.
//   Ray             32 B
//   RayHit          48 B
// The radiance-query records (urt_radiance_query, urt.h) likewise: three dwordx4 loads per ray, one 8-byte load per pixel.
//   PathRay         48 B
//   PathPixel        8 B
// The per-object motion entries of urt_reproject_objects (urt.h) are the library's own too: 48 bytes, three dwordx4 loads.
//   ObjectMotion    48 B
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma pack(push, 1)
typedef struct urt_RayTraceParams {
  float color_albedo[3];    /* @0  */
  float color_specular[3];  /* @12 */
  float emission[3];        /* @24 */
  float smoothness;         /* @36 */
} urt_RayTraceParams;

typedef struct urt_MeshObject {
  float localToWorldMatrix[16]; /* @0  Unity Matrix4x4 memory order = column-major m[col*4+row] */
  int32_t indices_offset;       /* @64 first slot of this mesh in _Indices */
  int32_t indices_count;        /* @68 number of index slots (3 per triangle) */
  urt_RayTraceParams lighting;  /* @72 */
} urt_MeshObject;

typedef struct urt_Sphere {
  float position[3];            /* @0  */
  float radius;                 /* @12 */
  urt_RayTraceParams lighting;  /* @16 */
} urt_Sphere;

typedef struct urt_BVHNode {
  float vmin[3];                /* @0  */
  float vmax[3];                /* @12 */
  int32_t index;                /* @24 <0: interior/filler, >=0: object id (implicit heap 2i+1, 2i+2) */
} urt_BVHNode;

typedef struct urt_Ray {
  float origin[3];              /* @0  */
  float t_max;                  /* @12 a hit counts only if 0 < t < t_max (exclusive; NaN or <= 0: no hit) */
  float direction[3];           /* @16 used as given (not normalised): distance is in units of |direction| */
  int32_t reserved;             /* @28 */
} urt_Ray;

typedef struct urt_RayHit {
  float distance;               /* @0  +inf: miss */
  float position[3];            /* @4  origin + distance * direction */
  float normal[3];              /* @16 */
  int32_t kind;                 /* @28 0 miss, 1 ground plane, 2 sphere, 3 triangle */
  int32_t object;               /* @32 sphere index or MeshObject index; -1 for a miss or the ground plane */
  int32_t primitive;            /* @36 triangle: its first index slot in _Indices (i of RS:243); -1 otherwise */
  float u, v;                   /* @40 triangle: barycentrics of the hit; 0 otherwise */
} urt_RayHit;

typedef struct urt_PathRay {
  float origin[3];              /* @0  */
  float seed;                   /* @12 the running _Seed the path's first rand() starts from (RS:16) */
  float direction[3];           /* @16 used as given (not normalised), as urt_Ray's */
  int32_t reserved0;            /* @28 */
  float px, py;                 /* @32 the "pixel" of rand() (RS:77-81): two finite floats, they select the query's random stream.  Any
                                       sign, fractions included, as long as  |a * d| * 0.6366 < 2^30  for every rand() of the query, with
                                       a = (seed + seed / 17) / 100, d = px * 12.9898 + py * 78.233 (urt_math.h rand_next) and the seed
                                       growing by 0.5 per draw: beyond that f_sincos's (int)k is not defined on the host.  |px|, |py| <=
                                       4096 with |seed| <= 64 is well inside */
  int32_t reserved1[2];         /* @40 */
} urt_PathRay;

typedef struct urt_PathPixel {
  int32_t x, y;                 /* @0, @4: pixel (x, y) of the texture bound as Result, row 0 at the bottom */
} urt_PathPixel;

typedef struct urt_ObjectMotion {
  float a[12];                  /* @0  current world -> previous world, affine: columns of the linear part a[0..2], a[3..5], a[6..8], then
                                       the translation a[9..11]:  P'.r = ((a[r]*P.x + a[3+r]*P.y) + a[6+r]*P.z) + a[9+r],  r = 0..2 */
} urt_ObjectMotion;
#pragma pack(pop)

#define URT_STRIDE_PARAMS 40
#define URT_STRIDE_MESHOBJECT 112
#define URT_STRIDE_SPHERE 56
#define URT_STRIDE_BVHNODE 28
#define URT_STRIDE_VEC3 12
#define URT_STRIDE_INDEX 4
#define URT_STRIDE_RAY 32
#define URT_STRIDE_RAYHIT 48
#define URT_STRIDE_OBJECTMOTION 48
#define URT_STRIDE_PATHRAY 48
#define URT_STRIDE_PATHPIXEL 8

#ifdef __cplusplus
}
static_assert(sizeof(urt_RayTraceParams) == URT_STRIDE_PARAMS, "RM:42");
static_assert(sizeof(urt_MeshObject) == URT_STRIDE_MESHOBJECT, "RM:43");
static_assert(sizeof(urt_Sphere) == URT_STRIDE_SPHERE, "RM:44");
static_assert(sizeof(urt_BVHNode) == URT_STRIDE_BVHNODE, "RM:45");
static_assert(sizeof(urt_Ray) == URT_STRIDE_RAY, "urt_Ray");
static_assert(sizeof(urt_RayHit) == URT_STRIDE_RAYHIT, "urt_RayHit");
static_assert(sizeof(urt_ObjectMotion) == URT_STRIDE_OBJECTMOTION, "urt_ObjectMotion");
static_assert(sizeof(urt_PathRay) == URT_STRIDE_PATHRAY, "urt_PathRay");
static_assert(sizeof(urt_PathPixel) == URT_STRIDE_PATHPIXEL, "urt_PathPixel");
#endif
