// Functional stand-in for the rclcpp / pluginlib / message surface that the reference's rollout units touch.
// Written from the libraries' documented behaviour; it includes and calls nothing under oracle/.
// rclcpp: parameter declare/get and logging only.  pluginlib: the export macro and a class loader.
#ifndef REF_SHIM_ROS_HPP_
#define REF_SHIM_ROS_HPP_
#include <cassert>
#include <chrono>
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace rclcpp {
enum ParameterType { PARAMETER_NOT_SET = 0, PARAMETER_BOOL, PARAMETER_INTEGER, PARAMETER_DOUBLE, PARAMETER_STRING,
                     PARAMETER_DOUBLE_ARRAY };

class ParameterValue {
 public:
  ParameterValue() = default;
  explicit ParameterValue(bool v) : type_(PARAMETER_BOOL), b_(v) {}
  explicit ParameterValue(int v) : type_(PARAMETER_INTEGER), i_(v) {}
  explicit ParameterValue(double v) : type_(PARAMETER_DOUBLE), d_(v) {}
  explicit ParameterValue(const char* v) : type_(PARAMETER_STRING), s_(v) {}
  explicit ParameterValue(const std::string& v) : type_(PARAMETER_STRING), s_(v) {}
  explicit ParameterValue(const std::vector<double>& v) : type_(PARAMETER_DOUBLE_ARRAY), a_(v) {}
  ParameterType get_type() const { return type_; }
  // rclcpp::Node::get_parameter(name, T&) converts the stored value to T; the driver always stores a parameter with the
  // type of the reference's default, so only same-kind conversions happen here.
  template <class T> T as() const {
    switch (type_) {
      case PARAMETER_BOOL: return static_cast<T>(b_);
      case PARAMETER_INTEGER: return static_cast<T>(i_);
      case PARAMETER_DOUBLE: return static_cast<T>(d_);
      default: throw std::runtime_error("ref shim: parameter is not a scalar");
    }
  }
  const std::vector<double>& as_double_array() const {
    if (type_ != PARAMETER_DOUBLE_ARRAY) throw std::runtime_error("ref shim: parameter is not a double array");
    return a_;
  }
  const std::string& as_string() const { return s_; }

 private:
  ParameterType type_ = PARAMETER_NOT_SET;
  bool b_ = false;
  long i_ = 0;
  double d_ = 0.0;
  std::string s_;
  std::vector<double> a_;
};

class Parameter {
 public:
  Parameter() = default;
  Parameter(std::string n, ParameterValue v) : name_(std::move(n)), v_(std::move(v)) {}
  const std::vector<double>& as_double_array() const { return v_.as_double_array(); }
  double as_double() const { return v_.as<double>(); }
  long as_int() const { return v_.as<long>(); }
  bool as_bool() const { return v_.as<bool>(); }
  const std::string& as_string() const { return v_.as_string(); }
  const std::string& get_name() const { return name_; }

 private:
  std::string name_;
  ParameterValue v_;
};

class Logger {
 public:
  Logger get_child(const std::string&) const { return *this; }
};

// rclcpp::Node reduced to its parameter map: declare_parameter returns the override when one is set (the driver plays
// the role of the launch file's parameter file), otherwise the default; get_parameter reads what was declared.
class Node {
 public:
  using SharedPtr = std::shared_ptr<Node>;
  using WeakPtr = std::weak_ptr<Node>;
  explicit Node(const std::string& name = "ref") : name_(name) {}
  void set_override(const std::string& n, ParameterValue v) { overrides_[n] = std::move(v); }
  const ParameterValue& declare_parameter(const std::string& n, const ParameterValue& dflt) {
    auto it = overrides_.find(n);
    declared_[n] = it != overrides_.end() ? it->second : dflt;
    return declared_[n];
  }
  const ParameterValue& declare_parameter(const std::string& n, ParameterType) {
    auto it = overrides_.find(n);
    declared_[n] = it != overrides_.end() ? it->second : ParameterValue();
    return declared_[n];
  }
  template <class T> bool get_parameter(const std::string& n, T& out) const {
    auto it = declared_.find(n);
    if (it == declared_.end()) return false;
    out = it->second.template as<T>();
    return true;
  }
  bool get_parameter(const std::string& n, std::string& out) const {
    auto it = declared_.find(n);
    if (it == declared_.end()) return false;
    out = it->second.as_string();
    return true;
  }
  Parameter get_parameter(const std::string& n) const {
    auto it = declared_.find(n);
    if (it == declared_.end()) throw std::runtime_error("ref shim: parameter not declared: " + n);
    return Parameter(n, it->second);
  }
  Logger get_logger() const { return Logger(); }
  const std::string& get_name() const { return name_; }

 private:
  std::string name_;
  std::map<std::string, ParameterValue> overrides_, declared_;
};

namespace node_interfaces {
class NodeLoggingInterface {
 public:
  using SharedPtr = std::shared_ptr<NodeLoggingInterface>;
  Logger get_logger() const { return Logger(); }
};
// NodeParametersInterface over a Node's parameter map (the launch file's role is Node::set_override, as above)
class NodeParametersInterface {
 public:
  using SharedPtr = std::shared_ptr<NodeParametersInterface>;
  explicit NodeParametersInterface(Node::SharedPtr node) : node_(std::move(node)) {}
  const ParameterValue& declare_parameter(const std::string& n, const ParameterValue& dflt) {
    return node_->declare_parameter(n, dflt);
  }
  Parameter get_parameter(const std::string& n) const { return node_->get_parameter(n); }

 private:
  Node::SharedPtr node_;
};
}  // namespace node_interfaces
struct Time { double s = 0.0; };
}  // namespace rclcpp

// Logging does nothing: the arguments are not evaluated (the reference's log arguments have no side effects).
// Except RCLCPP_DEBUG in a library built with -DREF_SHIM_TRACE_DEBUG: each call appends one record to a per-thread
// buffer, the number of its numeric arguments and then those arguments widened to double (the logger, the format and
// any non-numeric argument are dropped), so a driver reads a function's intermediate values where the reference logs
// them, without a change to the reference's text.  No ASSUMPTIONS.md row: nothing of rclcpp's arithmetic is involved.
namespace ref_shim_trace {
inline std::vector<double>& buffer() {
  static thread_local std::vector<double> b;
  return b;
}
template <class T> inline void put(std::vector<double>& b, std::size_t& n, const T& v) {
  if constexpr (std::is_arithmetic_v<T>) {
    b.push_back(static_cast<double>(v));
    ++n;
  }
}
template <class... A> inline void record(const char*, const A&... a) {
  std::vector<double>& b = buffer();
  const std::size_t at = b.size();
  std::size_t n = 0;
  b.push_back(0.0);
  (put(b, n, a), ...);
  b[at] = static_cast<double>(n);
}
}  // namespace ref_shim_trace
#ifdef REF_SHIM_TRACE_DEBUG
#define RCLCPP_DEBUG(logger, ...) ::ref_shim_trace::record(__VA_ARGS__)
#else
#define RCLCPP_DEBUG(...) do {} while (0)
#endif
#define RCLCPP_INFO(...) do {} while (0)
#define RCLCPP_WARN(...) do {} while (0)
#define RCLCPP_ERROR(...) do {} while (0)
#define RCLCPP_FATAL(...) do {} while (0)

// ---- messages: plain aggregates with the ROS 2 default values (Quaternion w = 1) ----
namespace std_msgs { namespace msg {
struct Header { rclcpp::Time stamp; std::string frame_id; };
} }
namespace geometry_msgs { namespace msg {
struct Vector3 { double x = 0.0, y = 0.0, z = 0.0; };
struct Point { double x = 0.0, y = 0.0, z = 0.0; };
struct Quaternion { double x = 0.0, y = 0.0, z = 0.0, w = 1.0; };
struct Pose { Point position; Quaternion orientation; };
struct PoseStamped { std_msgs::msg::Header header; Pose pose; };
struct Transform { Vector3 translation; Quaternion rotation; };
struct TransformStamped { std_msgs::msg::Header header; std::string child_frame_id; Transform transform; };
struct Twist { Vector3 linear, angular; };
struct TwistWithCovariance { Twist twist; double covariance[36] = {}; };
struct PoseWithCovariance { Pose pose; double covariance[36] = {}; };
} }
namespace nav_msgs { namespace msg {
struct Path { std_msgs::msg::Header header; std::vector<geometry_msgs::msg::PoseStamped> poses; };
struct Odometry { std_msgs::msg::Header header; std::string child_frame_id; geometry_msgs::msg::PoseWithCovariance pose;
                  geometry_msgs::msg::TwistWithCovariance twist; };
} }
namespace tf2_ros { class Buffer {}; }

// ---- pluginlib: PLUGINLIB_EXPORT_CLASS registers a factory under the plugin's type name ("ns::Class", as the
// plugin description XML names it); ClassLoader::createSharedInstance looks it up. ----
namespace pluginlib {
template <class Base> std::map<std::string, std::function<std::shared_ptr<Base>()>>& registry() {
  static std::map<std::string, std::function<std::shared_ptr<Base>()>> r;
  return r;
}
template <class Derived, class Base> struct Registrar {
  explicit Registrar(const char* type) { registry<Base>()[type] = [] { return std::make_shared<Derived>(); }; }
};
template <class Base> class ClassLoader {
 public:
  ClassLoader(const std::string&, const std::string&) {}
  std::shared_ptr<Base> createSharedInstance(const std::string& type) {
    auto it = registry<Base>().find(type);
    if (it == registry<Base>().end()) throw std::runtime_error("ref shim: no plugin " + type);
    return it->second();
  }
};
}  // namespace pluginlib
#define REF_PLUGINLIB_CAT2(a, b) a##b
#define REF_PLUGINLIB_CAT(a, b) REF_PLUGINLIB_CAT2(a, b)
#define PLUGINLIB_EXPORT_CLASS(Derived, Base) \
  static ::pluginlib::Registrar<Derived, Base> REF_PLUGINLIB_CAT(ref_plugin_registrar_, __LINE__)(#Derived);
#endif
