/*
 * oracle/shim/json/json.h — TEST INFRASTRUCTURE, our own code.
 *
 * A stand-in for the part of jsoncpp that the reference's example driver
 * (the .cpp files of examples/example1/src) uses, so that the driver compiles as it stands and the
 * project's data path can be held to it (oracle/build_ref.sh, oracle/driver_ref_harness.cpp).
 * Nothing here is taken from jsoncpp; only its public names and documented behaviour are
 * followed.  The surface, and nothing beyond it:
 *
 *   Json::Value      constructors (null, ValueType, int, double, const char*, std::string),
 *                    get(key, default), operator[] (int / string key, const and not),
 *                    append, size, empty, isNull, isArray, isObject, asInt, asDouble, asString,
 *                    operator==, range-for over arrays
 *   Json::Path       Path(".a.b").resolve(root) and .resolve(root, default)
 *   Json::CharReaderBuilder / CharReader::parse
 *   Json::StreamWriterBuilder (operator[], settings_) / StreamWriter::write
 *   JSONCPP_STRING
 *
 * PARSER.  Objects, arrays, strings with the usual escapes (\uXXXX to UTF-8, surrogate pairs
 * included), true / false / null and numbers; `//` and C comments are skipped and anything
 * behind the root value is ignored, as jsoncpp's default builder settings have it.  An integer
 * literal that fits 64 bits is kept as an integer; any other number goes through strtod, which
 * like the classic-locale stream jsoncpp reads through is correctly rounded on glibc.
 *
 * FOLLOWED ON PAPER ONLY.  These follow jsoncpp's documentation and could not be checked
 * against a real jsoncpp; the tests of this project must not depend on them:
 *   - null.asDouble() == 0.0, null.asInt() == 0, null.asString() == ""
 *   - bool converts to 0 / 1, a real converts to int by truncation when it is in range,
 *     a number's asString() is some text of it
 *   - operator[](int) on a non-const array beyond its end extends it with nulls;
 *     on a const value it yields null
 *   - get() and operator[](key) on null yield the default / null; on another non-object they throw
 *   - range-for over anything but an array visits nothing (jsoncpp visits an object's members)
 *   - the writer's text: valid JSON, members in key order, numbers with 17 significant digits;
 *     jsoncpp's own number formatting ("precision", "precisionType") is not reproduced
 */
#pragma once

#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#define JSONCPP_STRING std::string

namespace Json {

enum ValueType { nullValue = 0, intValue, uintValue, realValue, stringValue, booleanValue, arrayValue, objectValue };

class LogicError : public std::logic_error {
 public:
  explicit LogicError(const std::string& m) : std::logic_error(m) {}
};

class Value {
 public:
  using Members = std::map<std::string, Value>;
  using const_iterator = std::vector<Value>::const_iterator;

  Value(ValueType t = nullValue) : type_(t) {}
  Value(int v) : type_(intValue), int_(v) {}
  Value(double v) : type_(realValue), real_(v) {}
  Value(const char* s) : type_(stringValue), str_(s ? s : "") {}
  Value(const std::string& s) : type_(stringValue), str_(s) {}

  static Value makeBool(bool b) {
    Value v(booleanValue);
    v.int_ = b ? 1 : 0;
    return v;
  }
  static Value makeInt64(long long i) {
    Value v(intValue);
    v.int_ = i;
    return v;
  }

  ValueType type() const { return type_; }
  bool isNull() const { return type_ == nullValue; }
  bool isArray() const { return type_ == arrayValue; }
  bool isObject() const { return type_ == objectValue; }

  unsigned size() const {
    if (type_ == arrayValue) return static_cast<unsigned>(arr_.size());
    if (type_ == objectValue) return static_cast<unsigned>(obj_.size());
    return 0;
  }
  bool empty() const { return (isNull() || isArray() || isObject()) ? size() == 0 : false; }

  int asInt() const {
    switch (type_) {
      case nullValue: return 0;
      case booleanValue: return int_ ? 1 : 0;
      case intValue:
      case uintValue:
        if (int_ < INT_MIN || int_ > INT_MAX) throw LogicError("integer out of Int range");
        return static_cast<int>(int_);
      case realValue:
        if (!(real_ >= INT_MIN && real_ <= INT_MAX)) throw LogicError("double out of Int range");
        return static_cast<int>(real_);
      default: throw LogicError("Value is not convertible to Int.");
    }
  }
  double asDouble() const {
    switch (type_) {
      case nullValue: return 0.0;
      case booleanValue: return int_ ? 1.0 : 0.0;
      case intValue:
      case uintValue: return static_cast<double>(int_);
      case realValue: return real_;
      default: throw LogicError("Value is not convertible to double.");
    }
  }
  std::string asString() const {
    switch (type_) {
      case nullValue: return "";
      case stringValue: return str_;
      case booleanValue: return int_ ? "true" : "false";
      case intValue:
      case uintValue: return std::to_string(int_);
      case realValue: return realText(real_);
      default: throw LogicError("Type is not convertible to string");
    }
  }

  Value get(const char* key, const Value& def) const { return get(std::string(key), def); }
  Value get(const std::string& key, const Value& def) const {
    if (type_ == nullValue) return def;
    if (type_ != objectValue) throw LogicError("Value::get(key, default) requires an object or null");
    auto it = obj_.find(key);
    return it == obj_.end() ? def : it->second;
  }

  Value& operator[](int i) {
    if (type_ == nullValue) type_ = arrayValue;
    if (type_ != arrayValue || i < 0) throw LogicError("Value::operator[](int) requires an array");
    if (static_cast<size_t>(i) >= arr_.size()) arr_.resize(static_cast<size_t>(i) + 1);
    return arr_[static_cast<size_t>(i)];
  }
  const Value& operator[](int i) const {
    if (type_ == nullValue) return null();
    if (type_ != arrayValue || i < 0) throw LogicError("Value::operator[](int) const requires an array");
    return static_cast<size_t>(i) < arr_.size() ? arr_[static_cast<size_t>(i)] : null();
  }
  Value& operator[](const std::string& key) {
    if (type_ == nullValue) type_ = objectValue;
    if (type_ != objectValue) throw LogicError("Value::operator[](key) requires an object");
    return obj_[key];
  }
  const Value& operator[](const std::string& key) const {
    if (type_ == nullValue) return null();
    if (type_ != objectValue) throw LogicError("Value::operator[](key) const requires an object");
    auto it = obj_.find(key);
    return it == obj_.end() ? null() : it->second;
  }
  Value& operator[](const char* key) { return (*this)[std::string(key)]; }
  const Value& operator[](const char* key) const { return (*this)[std::string(key)]; }

  Value& append(const Value& v) {
    if (type_ == nullValue) type_ = arrayValue;
    if (type_ != arrayValue) throw LogicError("Value::append requires an array");
    arr_.push_back(v);
    return arr_.back();
  }

  bool operator==(const Value& o) const {
    if (type_ != o.type_) return false;
    switch (type_) {
      case nullValue: return true;
      case booleanValue:
      case intValue:
      case uintValue: return int_ == o.int_;
      case realValue: return real_ == o.real_;
      case stringValue: return str_ == o.str_;
      case arrayValue: return arr_ == o.arr_;
      default: return obj_ == o.obj_;
    }
  }
  bool operator!=(const Value& o) const { return !(*this == o); }

  const_iterator begin() const { return arr_.begin(); }
  const_iterator end() const { return arr_.end(); }

  const Members& members() const { return obj_; }
  const std::string& text() const { return str_; }
  long long integer() const { return int_; }
  double real() const { return real_; }

  static std::string realText(double d) {
    if (!std::isfinite(d)) return "null";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", d);
    std::string s(buf);
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
    return s;
  }

 private:
  static const Value& null() {
    static const Value n;
    return n;
  }
  ValueType type_;
  long long int_ = 0;
  double real_ = 0.0;
  std::string str_;
  std::vector<Value> arr_;
  Members obj_;
};

/* ---- Path ------------------------------------------------------------------------------- */
class Path {
 public:
  explicit Path(const std::string& path) {
    size_t i = 0;
    while (i < path.size()) {
      if (path[i] == '.') {
        ++i;
        continue;
      }
      size_t j = path.find('.', i);
      if (j == std::string::npos) j = path.size();
      keys_.push_back(path.substr(i, j - i));
      i = j;
    }
  }
  Value resolve(const Value& root) const { return resolve(root, Value()); }
  Value resolve(const Value& root, const Value& def) const {
    const Value* node = &root;
    for (const auto& k : keys_) {
      if (!node->isObject()) return def;
      const auto& m = node->members();
      auto it = m.find(k);
      if (it == m.end()) return def;
      node = &it->second;
    }
    return *node;
  }

 private:
  std::vector<std::string> keys_;
};

/* ---- reader ----------------------------------------------------------------------------- */
class CharReader {
 public:
  virtual ~CharReader() = default;
  virtual bool parse(const char* begin, const char* end, Value* root, JSONCPP_STRING* errs) {
    p_ = begin;
    e_ = end;
    err_.clear();
    Value v;
    bool ok = false;
    try {
      ok = value(v, 0);
    } catch (const std::exception& ex) {
      err_ = ex.what();
    }
    if (!ok) {
      if (errs) *errs = err_.empty() ? std::string("syntax error") : err_;
      return false;
    }
    if (root) *root = v;
    return true;
  }

 private:
  const char* p_ = nullptr;
  const char* e_ = nullptr;
  std::string err_;

  bool fail(const char* what) {
    if (err_.empty()) err_ = what;
    return false;
  }
  void skip() {
    for (;;) {
      while (p_ < e_ && (*p_ == ' ' || *p_ == '\t' || *p_ == '\n' || *p_ == '\r')) ++p_;
      if (p_ + 1 < e_ && p_[0] == '/' && p_[1] == '/') {
        while (p_ < e_ && *p_ != '\n' && *p_ != '\r') ++p_;
      } else if (p_ + 1 < e_ && p_[0] == '/' && p_[1] == '*') {
        p_ += 2;
        while (p_ + 1 < e_ && !(p_[0] == '*' && p_[1] == '/')) ++p_;
        p_ = (p_ + 1 < e_) ? p_ + 2 : e_;
      } else {
        return;
      }
    }
  }
  bool word(const char* w) {
    size_t n = std::strlen(w);
    if (static_cast<size_t>(e_ - p_) < n || std::strncmp(p_, w, n) != 0) return fail("unknown literal");
    p_ += n;
    return true;
  }
  static void utf8(unsigned cp, std::string& out) {
    if (cp < 0x80) {
      out += static_cast<char>(cp);
    } else if (cp < 0x800) {
      out += static_cast<char>(0xC0 | (cp >> 6));
      out += static_cast<char>(0x80 | (cp & 0x3F));
    } else if (cp < 0x10000) {
      out += static_cast<char>(0xE0 | (cp >> 12));
      out += static_cast<char>(0x80 | ((cp >> 6) & 0x3F));
      out += static_cast<char>(0x80 | (cp & 0x3F));
    } else {
      out += static_cast<char>(0xF0 | (cp >> 18));
      out += static_cast<char>(0x80 | ((cp >> 12) & 0x3F));
      out += static_cast<char>(0x80 | ((cp >> 6) & 0x3F));
      out += static_cast<char>(0x80 | (cp & 0x3F));
    }
  }
  bool hex4(unsigned& cp) {
    if (e_ - p_ < 4) return fail("short \\u escape");
    cp = 0;
    for (int i = 0; i < 4; ++i) {
      char c = *p_++;
      cp <<= 4;
      if (c >= '0' && c <= '9') cp |= static_cast<unsigned>(c - '0');
      else if (c >= 'a' && c <= 'f') cp |= static_cast<unsigned>(c - 'a' + 10);
      else if (c >= 'A' && c <= 'F') cp |= static_cast<unsigned>(c - 'A' + 10);
      else return fail("bad \\u escape");
    }
    return true;
  }
  bool string(std::string& out) {
    ++p_; /* the opening quote */
    while (p_ < e_) {
      char c = *p_++;
      if (c == '"') return true;
      if (c != '\\') {
        out += c;
        continue;
      }
      if (p_ >= e_) break;
      c = *p_++;
      switch (c) {
        case '"': out += '"'; break;
        case '\\': out += '\\'; break;
        case '/': out += '/'; break;
        case 'b': out += '\b'; break;
        case 'f': out += '\f'; break;
        case 'n': out += '\n'; break;
        case 'r': out += '\r'; break;
        case 't': out += '\t'; break;
        case 'u': {
          unsigned cp;
          if (!hex4(cp)) return false;
          if (cp >= 0xD800 && cp <= 0xDBFF) {
            unsigned lo;
            if (e_ - p_ < 6 || p_[0] != '\\' || p_[1] != 'u') return fail("lone surrogate");
            p_ += 2;
            if (!hex4(lo)) return false;
            cp = 0x10000 + ((cp & 0x3FF) << 10) + (lo & 0x3FF);
          }
          utf8(cp, out);
          break;
        }
        default: return fail("bad escape in string");
      }
    }
    return fail("unterminated string");
  }
  bool number(Value& v) {
    const char* s = p_;
    bool integer = true;
    if (p_ < e_ && *p_ == '-') ++p_;
    const char* digits = p_;
    while (p_ < e_ && *p_ >= '0' && *p_ <= '9') ++p_;
    if (p_ == digits) return fail("not a number");
    if (p_ < e_ && *p_ == '.') {
      integer = false;
      ++p_;
      while (p_ < e_ && *p_ >= '0' && *p_ <= '9') ++p_;
    }
    if (p_ < e_ && (*p_ == 'e' || *p_ == 'E')) {
      integer = false;
      ++p_;
      if (p_ < e_ && (*p_ == '+' || *p_ == '-')) ++p_;
      const char* ex = p_;
      while (p_ < e_ && *p_ >= '0' && *p_ <= '9') ++p_;
      if (p_ == ex) return fail("exponent without digits");
    }
    const std::string txt(s, p_);
    if (integer) {
      errno = 0;
      char* endp = nullptr;
      long long i = std::strtoll(txt.c_str(), &endp, 10);
      if (errno == 0 && *endp == '\0') {
        v = Value::makeInt64(i);
        return true;
      }
    }
    v = Value(std::strtod(txt.c_str(), nullptr));
    return true;
  }
  bool value(Value& v, int depth) {
    if (depth > 1000) return fail("nested too deeply");
    skip();
    if (p_ >= e_) return fail("unexpected end of text");
    switch (*p_) {
      case '{': {
        ++p_;
        v = Value(objectValue);
        skip();
        if (p_ < e_ && *p_ == '}') {
          ++p_;
          return true;
        }
        for (;;) {
          skip();
          if (p_ >= e_ || *p_ != '"') return fail("member name expected");
          std::string key;
          if (!string(key)) return false;
          skip();
          if (p_ >= e_ || *p_ != ':') return fail("':' expected");
          ++p_;
          Value m;
          if (!value(m, depth + 1)) return false;
          v[key] = m;
          skip();
          if (p_ < e_ && *p_ == ',') {
            ++p_;
            continue;
          }
          if (p_ < e_ && *p_ == '}') {
            ++p_;
            return true;
          }
          return fail("',' or '}' expected");
        }
      }
      case '[': {
        ++p_;
        v = Value(arrayValue);
        skip();
        if (p_ < e_ && *p_ == ']') {
          ++p_;
          return true;
        }
        for (;;) {
          Value m;
          if (!value(m, depth + 1)) return false;
          v.append(m);
          skip();
          if (p_ < e_ && *p_ == ',') {
            ++p_;
            continue;
          }
          if (p_ < e_ && *p_ == ']') {
            ++p_;
            return true;
          }
          return fail("',' or ']' expected");
        }
      }
      case '"': {
        std::string s;
        if (!string(s)) return false;
        v = Value(s);
        return true;
      }
      case 't':
        if (!word("true")) return false;
        v = Value::makeBool(true);
        return true;
      case 'f':
        if (!word("false")) return false;
        v = Value::makeBool(false);
        return true;
      case 'n':
        if (!word("null")) return false;
        v = Value();
        return true;
      default: return number(v);
    }
  }
};

class CharReaderBuilder {
 public:
  CharReader* newCharReader() const { return new CharReader; }
  Value settings_;
};

/* ---- writer ----------------------------------------------------------------------------- */
class StreamWriter {
 public:
  explicit StreamWriter(std::string indent = "\t") : indent_(std::move(indent)) {}
  virtual ~StreamWriter() = default;
  virtual int write(const Value& root, std::ostream* sout) {
    put(root, *sout, 0);
    return 0;
  }

 private:
  std::string indent_;
  void nl(std::ostream& o, int level) const {
    if (indent_.empty()) return;
    o << '\n';
    for (int i = 0; i < level; ++i) o << indent_;
  }
  static void quoted(const std::string& s, std::ostream& o) {
    o << '"';
    for (unsigned char c : s) {
      if (c == '"') o << "\\\"";
      else if (c == '\\') o << "\\\\";
      else if (c == '\n') o << "\\n";
      else if (c == '\r') o << "\\r";
      else if (c == '\t') o << "\\t";
      else if (c < 0x20) {
        char buf[8];
        std::snprintf(buf, sizeof buf, "\\u%04x", c);
        o << buf;
      } else o << static_cast<char>(c);
    }
    o << '"';
  }
  void put(const Value& v, std::ostream& o, int level) const {
    switch (v.type()) {
      case nullValue: o << "null"; break;
      case booleanValue: o << (v.integer() ? "true" : "false"); break;
      case intValue:
      case uintValue: o << v.integer(); break;
      case realValue: o << Value::realText(v.real()); break;
      case stringValue: quoted(v.text(), o); break;
      case arrayValue: {
        if (v.size() == 0) {
          o << "[]";
          break;
        }
        o << '[';
        bool first = true;
        for (const auto& e : v) {
          if (!first) o << ',';
          first = false;
          nl(o, level + 1);
          put(e, o, level + 1);
        }
        nl(o, level);
        o << ']';
        break;
      }
      default: {
        if (v.size() == 0) {
          o << "{}";
          break;
        }
        o << '{';
        bool first = true;
        for (const auto& kv : v.members()) {
          if (!first) o << ',';
          first = false;
          nl(o, level + 1);
          quoted(kv.first, o);
          o << (indent_.empty() ? ":" : " : ");
          put(kv.second, o, level + 1);
        }
        nl(o, level);
        o << '}';
      }
    }
  }
};

class StreamWriterBuilder {
 public:
  Value& operator[](const std::string& key) { return settings_[key]; }
  StreamWriter* newStreamWriter() const {
    const Value ind = settings_.get("indentation", Value("\t"));
    return new StreamWriter(ind.asString());
  }
  Value settings_{objectValue};
};

}  // namespace Json
