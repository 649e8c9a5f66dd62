// Stand-in for <SFML/Graphics.hpp> -- TEST INFRASTRUCTURE ONLY.
//
// The reference's SphereWorld.cpp and World.cpp are compiled unmodified against this
// header (oracle/Makefile, target `ref`) so that the restatements in oracle/ and tests/
// can be compared with the reference's own arithmetic.  It is written by hand from the
// documented behaviour of SFML 2.4.2 and holds only the surface those two files use:
// containers and no-op graphics objects.  No arithmetic of the reference lives here.
//
// What serves the drivers (oracle/ref/*_ref_main.cpp) and is not SFML, each marked below:
//   * Image::getPixel outside the image does not index memory (SFML would: it has no
//     bounds check); it raises sf::standin::outside_read and returns a sentinel colour;
//   * Image::setPixel stores that flag beside the pixel and clears it, so a frame carries
//     one flag per pixel; Image::assign fills an image from a decoded asset;
//   * Shader::setUniform records (name, value) into sf::standin::uniforms.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include <string>
#include <vector>

// The reference spells these the MSVC way; MSVC's <cmath> has them in std, libstdc++'s may not.
namespace std {
using ::asinf;
using ::fmodf;
using ::sqrtf;
}  // namespace std

namespace sf {

typedef unsigned char Uint8;  // SFML/Config.hpp: 8-bit unsigned integer

template <typename T>
struct Vector2 {
  Vector2() : x(0), y(0) {}                    // Vector2(): (0, 0)
  Vector2(T X, T Y) : x(X), y(Y) {}            // Vector2(X, Y)
  template <typename U>
  explicit Vector2(const Vector2<U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}  // static_cast per component
  T x;  // X coordinate
  T y;  // Y coordinate
};
template <typename T> Vector2<T> operator-(const Vector2<T>& r) { return Vector2<T>(-r.x, -r.y); }                        // memberwise negation
template <typename T> Vector2<T>& operator+=(Vector2<T>& l, const Vector2<T>& r) { l.x += r.x; l.y += r.y; return l; }    // memberwise +=
template <typename T> Vector2<T>& operator-=(Vector2<T>& l, const Vector2<T>& r) { l.x -= r.x; l.y -= r.y; return l; }    // memberwise -=
template <typename T> Vector2<T> operator+(const Vector2<T>& l, const Vector2<T>& r) { return Vector2<T>(l.x + r.x, l.y + r.y); }  // memberwise +
template <typename T> Vector2<T> operator-(const Vector2<T>& l, const Vector2<T>& r) { return Vector2<T>(l.x - r.x, l.y - r.y); }  // memberwise -
template <typename T> Vector2<T> operator*(const Vector2<T>& l, T r) { return Vector2<T>(l.x * r, l.y * r); }             // memberwise * scalar
template <typename T> Vector2<T> operator*(T l, const Vector2<T>& r) { return Vector2<T>(r.x * l, r.y * l); }             // scalar * memberwise (r.x * l)
template <typename T> Vector2<T>& operator*=(Vector2<T>& l, T r) { l.x *= r; l.y *= r; return l; }                       // memberwise *=
template <typename T> Vector2<T> operator/(const Vector2<T>& l, T r) { return Vector2<T>(l.x / r, l.y / r); }             // memberwise / scalar
template <typename T> Vector2<T>& operator/=(Vector2<T>& l, T r) { l.x /= r; l.y /= r; return l; }                       // memberwise /=
template <typename T> bool operator==(const Vector2<T>& l, const Vector2<T>& r) { return (l.x == r.x) && (l.y == r.y); }  // strict memberwise ==
template <typename T> bool operator!=(const Vector2<T>& l, const Vector2<T>& r) { return (l.x != r.x) || (l.y != r.y); }  // strict memberwise !=
typedef Vector2<int> Vector2i;           // Vector2<int>
typedef Vector2<unsigned int> Vector2u;  // Vector2<unsigned int>
typedef Vector2<float> Vector2f;         // Vector2<float>

template <typename T>
struct Vector3 {
  Vector3() : x(0), y(0), z(0) {}                   // Vector3(): (0, 0, 0)
  Vector3(T X, T Y, T Z) : x(X), y(Y), z(Z) {}      // Vector3(X, Y, Z)
  template <typename U>
  explicit Vector3(const Vector3<U>& v)             // static_cast per component
      : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
  T x;  // X coordinate
  T y;  // Y coordinate
  T z;  // Z coordinate
};
template <typename T> Vector3<T> operator-(const Vector3<T>& l) { return Vector3<T>(-l.x, -l.y, -l.z); }                                  // memberwise negation
template <typename T> Vector3<T>& operator+=(Vector3<T>& l, const Vector3<T>& r) { l.x += r.x; l.y += r.y; l.z += r.z; return l; }        // memberwise +=
template <typename T> Vector3<T>& operator-=(Vector3<T>& l, const Vector3<T>& r) { l.x -= r.x; l.y -= r.y; l.z -= r.z; return l; }        // memberwise -=
template <typename T> Vector3<T> operator+(const Vector3<T>& l, const Vector3<T>& r) { return Vector3<T>(l.x + r.x, l.y + r.y, l.z + r.z); }  // memberwise +
template <typename T> Vector3<T> operator-(const Vector3<T>& l, const Vector3<T>& r) { return Vector3<T>(l.x - r.x, l.y - r.y, l.z - r.z); }  // memberwise -
template <typename T> Vector3<T> operator*(const Vector3<T>& l, T r) { return Vector3<T>(l.x * r, l.y * r, l.z * r); }                    // memberwise * scalar
template <typename T> Vector3<T> operator*(T l, const Vector3<T>& r) { return Vector3<T>(r.x * l, r.y * l, r.z * l); }                    // scalar * memberwise (r.x * l)
template <typename T> Vector3<T>& operator*=(Vector3<T>& l, T r) { l.x *= r; l.y *= r; l.z *= r; return l; }                              // memberwise *=
template <typename T> Vector3<T> operator/(const Vector3<T>& l, T r) { return Vector3<T>(l.x / r, l.y / r, l.z / r); }                    // memberwise / scalar
template <typename T> Vector3<T>& operator/=(Vector3<T>& l, T r) { l.x /= r; l.y /= r; l.z /= r; return l; }                              // memberwise /=
template <typename T> bool operator==(const Vector3<T>& l, const Vector3<T>& r) { return (l.x == r.x) && (l.y == r.y) && (l.z == r.z); }  // strict memberwise ==
template <typename T> bool operator!=(const Vector3<T>& l, const Vector3<T>& r) { return (l.x != r.x) || (l.y != r.y) || (l.z != r.z); }  // strict memberwise !=
typedef Vector3<int> Vector3i;    // Vector3<int>
typedef Vector3<float> Vector3f;  // Vector3<float>

struct Color {
  Color() : r(0), g(0), b(0), a(255) {}                                                      // Color(): opaque black
  Color(Uint8 red, Uint8 green, Uint8 blue, Uint8 alpha = 255) : r(red), g(green), b(blue), a(alpha) {}  // alpha defaults to 255
  static const Color Black;  // Color::Black: (0, 0, 0, 255)
  Uint8 r;  // red
  Uint8 g;  // green
  Uint8 b;  // blue
  Uint8 a;  // alpha (opacity)
};
inline const Color Color::Black(0, 0, 0, 255);

namespace Glsl {
struct Vec4 {  // Glsl::Vec4 is priv::Vector4<float>
  Vec4() : x(0), y(0), z(0), w(0) {}                                      // Vector4(): zeros
  Vec4(float X, float Y, float Z, float W) : x(X), y(Y), z(Z), w(W) {}    // Vector4(X, Y, Z, W)
  float x;  // 1st component
  float y;  // 2nd component
  float z;  // 3rd component
  float w;  // 4th component
};
}  // namespace Glsl

namespace standin {  // not SFML: what the drivers read back
inline int outside_read = 0;                          // raised by Image::getPixel outside the image
inline const Color outside_colour(255, 0, 255, 255);  // what such a read returns (the restatements' magenta)
struct Uniform {
  std::string name;
  int kind;    // 0 Glsl::Vec4, 1 int, 2 float, 3 Texture
  float v[4];
  int i;
};
inline std::vector<Uniform> uniforms;                 // every Shader::setUniform call, in call order
}  // namespace standin

class Image {
 public:
  void create(unsigned int width, unsigned int height, const Color& color = Color(0, 0, 0)) {  // fills with `color`
    w_ = width;
    h_ = height;
    px_.assign(static_cast<std::size_t>(width) * height * 4, 0);
    flags_.assign(static_cast<std::size_t>(width) * height, 0);
    for (std::size_t k = 0; k < px_.size(); k += 4) {
      px_[k] = color.r; px_[k + 1] = color.g; px_[k + 2] = color.b; px_[k + 3] = color.a;
    }
  }
  bool loadFromFile(const std::string& filename);           // decodes to RGBA8; defined by each driver
  Vector2u getSize() const { return Vector2u(w_, h_); }     // size in pixels
  // SFML reads m_pixels[(x + y * width) * 4] in unsigned arithmetic with no bounds check; an
  // index at or past width * height is the "read outside a texture" flagged here.
  Color getPixel(unsigned int x, unsigned int y) const {
    const unsigned int idx = x + y * w_;
    if (idx >= w_ * h_) {
      standin::outside_read = 1;
      return standin::outside_colour;
    }
    const Uint8* p = &px_[static_cast<std::size_t>(idx) * 4];
    return Color(p[0], p[1], p[2], p[3]);
  }
  void setPixel(unsigned int x, unsigned int y, const Color& color) {  // writes m_pixels[(x + y * width) * 4 ..]
    const unsigned int idx = x + y * w_;
    if (idx >= w_ * h_) return;  // SFML: undefined; the drivers never do it
    Uint8* p = &px_[static_cast<std::size_t>(idx) * 4];
    p[0] = color.r; p[1] = color.g; p[2] = color.b; p[3] = color.a;
    // not SFML: UpdateImage stores each ray's colour right after tracing it, so the flag a
    // read raised since the last store belongs to this pixel
    if (!flags_.empty()) flags_[idx] = static_cast<Uint8>(standin::outside_read);
    standin::outside_read = 0;
  }
  const Uint8* getFlagsPtr() const { return flags_.empty() ? nullptr : flags_.data(); }  // not SFML: per-pixel outside-read flags
  const Uint8* getPixelsPtr() const { return px_.empty() ? nullptr : px_.data(); }  // row-major RGBA8
  // not SFML: the drivers fill an image from a decoded asset
  void assign(unsigned int width, unsigned int height, const Uint8* rgba) {
    w_ = width;
    h_ = height;
    px_.assign(rgba, rgba + static_cast<std::size_t>(width) * height * 4);
  }

 private:
  unsigned int w_ = 0, h_ = 0;
  std::vector<Uint8> px_;     // row-major RGBA8
  std::vector<Uint8> flags_;  // not SFML: one outside-read flag per pixel of a created image
};

class Texture {
 public:
  bool loadFromFile(const std::string&) { return true; }  // GL upload: nothing to do here
  void setRepeated(bool) {}                               // GL sampler state
  bool generateMipmap() { return true; }                  // GL mipmaps
};

class Shader {
 public:
  enum Type { Vertex, Geometry, Fragment };                           // Shader::Type
  bool loadFromFile(const std::string&, Type) { return true; }        // GL compile: nothing to do here
  void setUniform(const std::string& name, float x) { standin::uniforms.push_back({name, 2, {x, 0, 0, 0}, 0}); }      // float uniform
  void setUniform(const std::string& name, int x) { standin::uniforms.push_back({name, 1, {0, 0, 0, 0}, x}); }        // int uniform
  void setUniform(const std::string& name, const Glsl::Vec4& v) { standin::uniforms.push_back({name, 0, {v.x, v.y, v.z, v.w}, 0}); }  // vec4 uniform
  void setUniform(const std::string& name, const Texture&) { standin::uniforms.push_back({name, 3, {0, 0, 0, 0}, 0}); }  // sampler2D uniform
};

class Clock {
 public:
  Clock() {}  // starts a timer the traced paths never read
};

}  // namespace sf
