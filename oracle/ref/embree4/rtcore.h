/*
 * Stand-in for <embree4/rtcore.h> -- TEST INFRASTRUCTURE ONLY (oracle/Makefile, target _ref/libhz_ref.so).
 *
 * Exactly the part of Embree 4's public C API that the reference's horizon_comp.cpp and shadow_comp.cpp name:
 * sixteen entry points, the handles, enums and structs they take.  Written from Embree's published API
 * documentation; the functions are implemented by oracle/ref/standin.cpp, which answers every ray with the
 * oracle's scene and triangle test (oracle/hz_oracle.c).  Nothing here ray-traces by itself.
 */
#ifndef HZ_REF_STANDIN_RTCORE_H
#define HZ_REF_STANDIN_RTCORE_H

#include <stddef.h>

#if defined(__cplusplus)
extern "C" {
#endif

typedef struct HzRefDevice *RTCDevice;
typedef struct HzRefScene *RTCScene;
typedef struct HzRefGeometry *RTCGeometry;

#define RTC_INVALID_GEOMETRY_ID ((unsigned int)-1)
#define RTC_MAX_INSTANCE_LEVEL_COUNT 1

enum RTCError {
    RTC_ERROR_NONE = 0,
    RTC_ERROR_UNKNOWN = 1,
    RTC_ERROR_INVALID_ARGUMENT = 2,
    RTC_ERROR_INVALID_OPERATION = 3,
    RTC_ERROR_OUT_OF_MEMORY = 4,
    RTC_ERROR_UNSUPPORTED_CPU = 5,
    RTC_ERROR_CANCELLED = 6
};

enum RTCSceneFlags {
    RTC_SCENE_FLAG_NONE = 0,
    RTC_SCENE_FLAG_DYNAMIC = 1 << 0,
    RTC_SCENE_FLAG_COMPACT = 1 << 1,
    RTC_SCENE_FLAG_ROBUST = 1 << 2
};

enum RTCGeometryType {
    RTC_GEOMETRY_TYPE_TRIANGLE = 0,
    RTC_GEOMETRY_TYPE_QUAD = 1,
    RTC_GEOMETRY_TYPE_GRID = 2
};

enum RTCBufferType {
    RTC_BUFFER_TYPE_INDEX = 0,
    RTC_BUFFER_TYPE_VERTEX = 1,
    RTC_BUFFER_TYPE_GRID = 8
};

enum RTCFormat {
    RTC_FORMAT_UNDEFINED = 0,
    RTC_FORMAT_UINT3 = 0x5003,
    RTC_FORMAT_UINT4 = 0x5004,
    RTC_FORMAT_FLOAT3 = 0x9003,
    RTC_FORMAT_GRID = 0xA001
};

struct RTCGrid {
    unsigned int startVertexID;
    unsigned int stride;
    unsigned short width, height;
};

struct RTCRay {
    float org_x, org_y, org_z, tnear;
    float dir_x, dir_y, dir_z, time;
    float tfar;
    unsigned int mask, id, flags;
};

struct RTCHit {
    float Ng_x, Ng_y, Ng_z;
    float u, v;
    unsigned int primID, geomID;
    unsigned int instID[RTC_MAX_INSTANCE_LEVEL_COUNT];
};

struct RTCRayHit {
    struct RTCRay ray;
    struct RTCHit hit;
};

struct RTCIntersectArguments;
struct RTCOccludedArguments;

typedef void (*RTCErrorFunction)(void *userPtr, enum RTCError code, const char *str);

RTCDevice rtcNewDevice(const char *config);
void rtcReleaseDevice(RTCDevice device);
enum RTCError rtcGetDeviceError(RTCDevice device);
void rtcSetDeviceErrorFunction(RTCDevice device, RTCErrorFunction error, void *userPtr);

RTCScene rtcNewScene(RTCDevice device);
void rtcSetSceneFlags(RTCScene scene, enum RTCSceneFlags flags);
void rtcCommitScene(RTCScene scene);
void rtcReleaseScene(RTCScene scene);

RTCGeometry rtcNewGeometry(RTCDevice device, enum RTCGeometryType type);
void rtcSetSharedGeometryBuffer(RTCGeometry geometry, enum RTCBufferType type, unsigned int slot,
                                enum RTCFormat format, const void *ptr, size_t byteOffset, size_t byteStride,
                                size_t itemCount);
void *rtcSetNewGeometryBuffer(RTCGeometry geometry, enum RTCBufferType type, unsigned int slot,
                              enum RTCFormat format, size_t byteStride, size_t itemCount);
void rtcCommitGeometry(RTCGeometry geometry);
unsigned int rtcAttachGeometry(RTCScene scene, RTCGeometry geometry);
void rtcReleaseGeometry(RTCGeometry geometry);

#if defined(__cplusplus)
void rtcIntersect1(RTCScene scene, struct RTCRayHit *rayhit, struct RTCIntersectArguments *args = NULL);
void rtcOccluded1(RTCScene scene, struct RTCRay *ray, struct RTCOccludedArguments *args = NULL);
#else
void rtcIntersect1(RTCScene scene, struct RTCRayHit *rayhit, struct RTCIntersectArguments *args);
void rtcOccluded1(RTCScene scene, struct RTCRay *ray, struct RTCOccludedArguments *args);
#endif

#if defined(__cplusplus)
}
#endif

#endif
