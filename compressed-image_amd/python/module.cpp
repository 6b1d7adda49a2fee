// python/module.cpp -- the `compressed_image` Python module: Codec, Channel, Image, mirroring the
// reference's pybind11 surface (python/py_module/compressed_image/_stubs/_compressed_image.pyi:11-306;
// bind_channel.h:17-255, bind_image.h:34-480, bind_enums.h:15-24) on top of the host mirror in
// ../include/compressed.  dtype -> T dispatch over the same nine element types as the reference's
// variant_t.h:92-103.  Out of scope here: Image.read / dtype(s)_from_file (OpenImageIO is absent).
// DeviceChannel / DeviceImage / DeviceArray (not in the reference): the same surface over compressed/device_channel.h and
// device_image.h, taking and filling GPU arrays through __cuda_array_interface__ -- neither torch nor HIP is linked here.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <variant>
#include <vector>

#include "compressed/channel.h"
#include "compressed/half.h"
#include "compressed/image.h"
#include "compressed/device_image.h"

namespace py = pybind11;
using compressed::enums::codec;

namespace
{
	template <typename... Ts> struct type_list {};
	using pixel_types = type_list<compressed::half, float, double, uint8_t, int8_t, uint16_t, int16_t, uint32_t, int32_t>;

	template <typename T> const char* dtype_code();
	template <> const char* dtype_code<compressed::half>() { return "float16"; }
	template <> const char* dtype_code<float>() { return "float32"; }
	template <> const char* dtype_code<double>() { return "float64"; }
	template <> const char* dtype_code<uint8_t>() { return "uint8"; }
	template <> const char* dtype_code<int8_t>() { return "int8"; }
	template <> const char* dtype_code<uint16_t>() { return "uint16"; }
	template <> const char* dtype_code<int16_t>() { return "int16"; }
	template <> const char* dtype_code<uint32_t>() { return "uint32"; }
	template <> const char* dtype_code<int32_t>() { return "int32"; }
	template <typename T> py::dtype np_dtype() { return py::dtype(dtype_code<T>()); }

	py::dtype as_dtype(const py::object& o) { return py::dtype::from_args(o); }

	// call f.template operator()<T>() for the T whose numpy dtype equals `dt`; ValueError otherwise
	template <typename F, typename... Ts>
	auto dispatch(const py::dtype& dt, F&& f, type_list<Ts...>)
	{
		using R = decltype(f.template operator()<uint8_t>());
		std::optional<R> out;
		const bool hit = ((dt.is(np_dtype<Ts>()) ? (out.emplace(f.template operator()<Ts>()), true) : false) || ...);
		if (!hit)
			throw py::value_error("Unsupported dtype '" + std::string(py::str(dt)) + "': supported are float16/32/64, (u)int8/16/32");
		return std::move(*out);
	}
	template <typename F> auto dispatch(const py::dtype& dt, F&& f) { return dispatch(dt, std::forward<F>(f), pixel_types{}); }

	template <typename T> T from_scalar(const py::object& v)
	{
		if constexpr (std::is_same_v<T, compressed::half>) return compressed::half(v.cast<double>());
		else if constexpr (std::is_floating_point_v<T>) return static_cast<T>(v.cast<double>());
		else return static_cast<T>(v.cast<long long>());
	}

	// value= of fill_region / fill_regions: a number (also a 0-d array), or -- where `many` > 0 -- a sequence or array of `many`
	// numbers (regions for channels, channels for images)
	template <typename T> std::vector<T> fill_values(const py::object& value, size_t many, const char* what)
	{
		const bool is_array = py::isinstance<py::array>(value);
		const bool seq = is_array ? py::reinterpret_borrow<py::array>(value).ndim() > 0
			: (py::isinstance<py::sequence>(value) && !py::isinstance<py::str>(value) && !py::isinstance<py::bytes>(value));
		std::vector<T> v;
		if (!seq) { v.push_back(from_scalar<T>(value)); return v; }
		if (many == 0) throw py::value_error(std::string(what) + ": value must be one number");
		for (auto h : value) v.push_back(from_scalar<T>(py::reinterpret_borrow<py::object>(h)));
		if (v.size() != 1 && v.size() != many)
			throw py::value_error(std::string(what) + ": value holds " + std::to_string(v.size()) + " numbers, expected one or " + std::to_string(many));
		return v;
	}
	// mask= / masks= of the host classes: a numpy array of dtype bool or uint8 and exactly `shape` (a contiguous copy is kept)
	inline std::pair<py::array, std::span<const uint8_t>> host_mask(const py::object& mask, const std::vector<py::ssize_t>& shape, const char* what)
	{
		if (!py::isinstance<py::array>(mask)) throw py::value_error(std::string(what) + ": a mask is a numpy array of dtype bool or uint8");
		py::array a = py::reinterpret_borrow<py::array>(mask);
		if (!a.dtype().is(py::dtype("uint8")) && !a.dtype().is(py::dtype("bool")))
			throw py::value_error(std::string(what) + ": a mask has dtype bool or uint8, got " + std::string(py::str(a.dtype())));
		if (std::vector<py::ssize_t>(a.shape(), a.shape() + a.ndim()) != shape)
			throw py::value_error(std::string(what) + ": the mask's shape does not match the written elements' shape");
		py::array c = py::module_::import("numpy").attr("ascontiguousarray")(a);
		return { c, std::span<const uint8_t>(static_cast<const uint8_t*>(c.data()), static_cast<size_t>(c.size())) };
	}

	// contiguous view of the array's elements as T (copying only if it is not C-contiguous)
	template <typename T> std::pair<py::array, std::span<const T>> elements(const py::array& a)
	{
		py::array c = py::array::ensure(a, py::array::c_style);
		if (!c) throw py::value_error("array is not convertible to a C-contiguous buffer");
		return { c, std::span<const T>(static_cast<const T*>(c.data()), static_cast<size_t>(c.size())) };
	}
	// Result arrays of get_decompressed() own a recycled page-locked buffer (compressed/detail/pinned_pool.h): the
	// engine's D2H copy lands in it by DMA and there are no first-touch page faults.  Dropping the array returns the
	// buffer to the pool.
	template <typename T> py::array pooled_array(std::vector<py::ssize_t> shape)
	{
		size_t count = 1;
		for (auto d : shape) count *= static_cast<size_t>(d);
		using pool = compressed::detail::pinned_pool;
		auto* s = new pool::block(pool::get().take(std::max<size_t>(count * sizeof(T), 1)));
		py::capsule owner(s, [](void* p) { auto* b = static_cast<pool::block*>(p); pool::get().give(*b); delete b; });
		return py::array(np_dtype<T>(), std::move(shape), s->p, owner);
	}

	template <typename T> py::array to_array(std::vector<T>&& pixels, std::vector<py::ssize_t> shape)
	{
		auto* heap = new std::vector<T>(std::move(pixels));
		py::capsule owner(heap, [](void* p) { delete static_cast<std::vector<T>*>(p); });
		return py::array(np_dtype<T>(), std::move(shape), heap->data(), owner);
	}

	// ---- subsampled regions and numpy-style keys ----------------------------------------------------------
	inline void check_steps(py::ssize_t step_x, py::ssize_t step_y)
	{
		if (step_x < 1 || step_y < 1) throw py::value_error("step_x and step_y must be >= 1");
	}
	inline py::ssize_t ceil_div(py::ssize_t a, py::ssize_t b) { return (a + b - 1) / b; }
	// the rectangle side that n samples `step` apart cover: (n - 1) * step + 1 (0 for none)
	inline size_t covered(py::ssize_t n, py::ssize_t step) { return n > 0 ? static_cast<size_t>((n - 1) * step + 1) : 0; }

	// one axis of a key: `count` elements from `start`, `step` apart; an integer drops its axis
	struct axis_pick { py::ssize_t start = 0, count = 0, step = 1; bool drop = false; };
	inline axis_pick pick_axis(const py::handle& k, py::ssize_t len)
	{
		axis_pick a;
		if (py::isinstance<py::slice>(k))
		{
			py::ssize_t start = 0, stop = 0, step = 1, n = 0;
			if (!py::reinterpret_borrow<py::slice>(k).compute(len, &start, &stop, &step, &n)) throw py::error_already_set();
			if (step < 1) throw py::value_error("negative slice steps are not supported");
			a.start = n > 0 ? start : 0; a.count = n; a.step = n > 1 ? step : 1;
			return a;
		}
		if (k.is_none()) throw py::type_error("None (numpy.newaxis) is not supported as an index");
		if (k.ptr() == Py_Ellipsis) throw py::type_error("Ellipsis is not supported as an index");
		if (py::isinstance<py::bool_>(k) || !PyIndex_Check(k.ptr()))
			throw py::type_error("indices must be integers or slices (index arrays, masks and lists are not supported)");
		const py::ssize_t i = PyNumber_AsSsize_t(k.ptr(), PyExc_IndexError);
		if (i == -1 && PyErr_Occurred()) throw py::error_already_set();
		if (i < -len || i >= len) throw py::index_error("index " + std::to_string(i) + " is out of bounds for an axis of size " + std::to_string(len));
		a.start = i < 0 ? i + len : i; a.count = 1; a.drop = true;
		return a;
	}

	// a[key] of a (height, width) channel as a strided region: the source rectangle, the steps and the result's shape
	struct region_pick { py::ssize_t x = 0, y = 0, w = 0, h = 0, sx = 1, sy = 1; std::vector<py::ssize_t> shape; };
	inline region_pick pick_region(const py::object& key, py::ssize_t height, py::ssize_t width)
	{
		py::object rk = key, ck = py::slice(py::none(), py::none(), py::none());
		if (py::isinstance<py::tuple>(key))
		{
			const py::tuple t = key;
			if (t.size() > 2) throw py::index_error("too many indices: a channel has 2 dimensions, " + std::to_string(t.size()) + " were indexed");
			rk = t.size() > 0 ? py::object(t[0]) : ck;
			if (t.size() > 1) ck = t[1];
		}
		const axis_pick r = pick_axis(rk, height), c = pick_axis(ck, width);
		region_pick p;
		p.y = r.start; p.sy = r.step; p.h = r.count > 0 ? (r.count - 1) * r.step + 1 : 0;
		p.x = c.start; p.sx = c.step; p.w = c.count > 0 ? (c.count - 1) * c.step + 1 : 0;
		if (!r.drop) p.shape.push_back(r.count);
		if (!c.drop) p.shape.push_back(c.count);
		return p;
	}

	// ---- batched reads: get_regions(xs, ys, width, height, step_x, step_y) and get_pixels(xs, ys) -------------------------
	// xs / ys: integer sequences or arrays of one length N (anything else: ValueError; a coordinate outside the image: IndexError)
	inline std::vector<py::ssize_t> coordinate_list(const py::object& o, const char* name)
	{
		py::array a = py::array::ensure(o);
		if (!a) { PyErr_Clear(); throw py::value_error(std::string(name) + " must be a sequence or an array of integers"); }
		if (a.ndim() != 1) throw py::value_error(std::string(name) + " must be one-dimensional");
		const char kind = a.dtype().kind();
		if (a.size() > 0 && kind != 'i' && kind != 'u') throw py::value_error(std::string(name) + " must hold integers, got dtype " + std::string(py::str(a.dtype())));
		py::array_t<int64_t, py::array::c_style | py::array::forcecast> v(a);
		std::vector<py::ssize_t> out(static_cast<size_t>(v.size()));
		for (size_t i = 0; i < out.size(); ++i) out[i] = static_cast<py::ssize_t>(v.data()[i]);
		return out;
	}
	inline std::vector<compressed::region> region_list(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height,
		py::ssize_t step_x, py::ssize_t step_y)
	{
		if (width < 0 || height < 0) throw py::value_error("region sizes must be >= 0");
		check_steps(step_x, step_y);
		const auto x = coordinate_list(xs, "xs"), y = coordinate_list(ys, "ys");
		if (x.size() != y.size()) throw py::value_error("xs and ys must have the same length, got " + std::to_string(x.size()) + " and " + std::to_string(y.size()));
		std::vector<compressed::region> r(x.size());
		for (size_t i = 0; i < r.size(); ++i)
		{
			if (x[i] < 0 || y[i] < 0) throw py::index_error("region " + std::to_string(i) + " starts at a negative coordinate");
			r[i] = compressed::region{ static_cast<size_t>(x[i]), static_cast<size_t>(y[i]), static_cast<size_t>(width), static_cast<size_t>(height),
				static_cast<size_t>(step_x), static_cast<size_t>(step_y) };
		}
		return r;
	}
	// the result's shape: (N, [C,] h', w') for get_regions, (N, [C]) for get_pixels
	inline std::vector<py::ssize_t> regions_shape(size_t n, std::optional<size_t> channels, py::ssize_t width, py::ssize_t height, py::ssize_t step_x,
		py::ssize_t step_y, bool pixels)
	{
		std::vector<py::ssize_t> shape{ static_cast<py::ssize_t>(n) };
		if (channels) shape.push_back(static_cast<py::ssize_t>(*channels));
		if (!pixels) { shape.push_back(ceil_div(height, step_y)); shape.push_back(ceil_div(width, step_x)); }
		return shape;
	}

	// ---- Channel ------------------------------------------------------------------------------------------
	template <typename T> using chan_ptr = std::shared_ptr<compressed::channel<T>>;
	using any_channel = std::variant<chan_ptr<compressed::half>, chan_ptr<float>, chan_ptr<double>, chan_ptr<uint8_t>, chan_ptr<int8_t>,
		chan_ptr<uint16_t>, chan_ptr<int16_t>, chan_ptr<uint32_t>, chan_ptr<int32_t>>;

	struct Channel
	{
		any_channel impl;

		template <typename F> auto visit(F&& f) const { return std::visit([&](auto& p) { return f(*p); }, impl); }

		// a[key] for key = a row index or slice, or a 2-tuple of those, as numpy has it (positive steps only)
		py::array getitem(const py::object& key) const
		{
			return visit([&]<typename T>(compressed::channel<T>& ch) {
				const region_pick p = pick_region(key, static_cast<py::ssize_t>(ch.height()), static_cast<py::ssize_t>(ch.width()));
				py::array out(np_dtype<T>(), p.shape);
				if (out.size() == 0) return out;
				ch.get_region(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(out.size())), static_cast<size_t>(p.x),
					static_cast<size_t>(p.y), static_cast<size_t>(p.w), static_cast<size_t>(p.h), static_cast<size_t>(p.sx), static_cast<size_t>(p.sy));
				return out;
			});
		}

		static Channel from_array(const py::array& data, size_t width, size_t height, codec c, size_t level, size_t block, size_t chunk, std::optional<int> mantissa)
		{
			return dispatch(data.dtype(), [&]<typename T>() {
				compressed::blosc2::ensure_mantissa_bits<T>(mantissa);          // (ValueError before anything else happens)
				auto [keep, px] = elements<T>(data);
				if (px.size() != width * height)
					throw py::value_error("Channel data has " + std::to_string(px.size()) + " elements, expected width * height = " + std::to_string(width * height));
				return Channel{ std::make_shared<compressed::channel<T>>(px, width, height, c, static_cast<uint8_t>(std::min<size_t>(level, 255)), block, chunk, mantissa) };
			});
		}
		static Channel full(const py::object& dtype, const py::object& fill, size_t width, size_t height, codec c, size_t level, size_t block, size_t chunk)
		{
			return dispatch(as_dtype(dtype), [&]<typename T>() {
				return Channel{ std::make_shared<compressed::channel<T>>(compressed::channel<T>::full(width, height, from_scalar<T>(fill), c,
					static_cast<uint8_t>(std::min<size_t>(level, 255)), block, chunk)) };
			});
		}
		static Channel full_like(const Channel& other, const py::object& fill)
		{
			return other.visit([&]<typename T>(compressed::channel<T>& ch) {
				return Channel{ std::make_shared<compressed::channel<T>>(compressed::channel<T>::full_like(ch, from_scalar<T>(fill))) };
			});
		}

		py::dtype dtype() const { return visit([]<typename T>(compressed::channel<T>&) { return np_dtype<T>(); }); }
		std::optional<int> mantissa_bits() const { return visit([](auto& c) { return c.mantissa_bits(); }); }
		size_t width() const { return visit([](auto& c) { return c.width(); }); }
		size_t height() const { return visit([](auto& c) { return c.height(); }); }

		py::array get_chunk(size_t index) const
		{
			return visit([&]<typename T>(compressed::channel<T>& ch) {
				if (index >= ch.num_chunks()) throw py::index_error("chunk index " + std::to_string(index) + " out of range, channel has " + std::to_string(ch.num_chunks()) + " chunks");
				std::vector<T> px(ch.chunk_elems(index));
				ch.get_chunk(std::span<T>(px), index);
				return to_array<T>(std::move(px), { static_cast<py::ssize_t>(ch.chunk_elems(index)) });
			});
		}
		py::array get_chunk_into(size_t index, py::array buffer) const
		{
			visit([&]<typename T>(compressed::channel<T>& ch) {
				if (index >= ch.num_chunks()) throw py::index_error("chunk index out of range");
				check_chunk_array<T>(buffer, ch.chunk_elems(index), /*exact=*/false);
				ch.get_chunk(std::span<T>(static_cast<T*>(buffer.mutable_data()), static_cast<size_t>(buffer.size())), index);
				return 0;
			});
			return buffer;
		}
		void set_chunk(size_t index, const py::array& array)
		{
			visit([&]<typename T>(compressed::channel<T>& ch) {
				if (index >= ch.num_chunks()) throw py::index_error("chunk index " + std::to_string(index) + " out of range, channel has " + std::to_string(ch.num_chunks()) + " chunks");
				check_chunk_array<T>(array, ch.chunk_elems(index), /*exact=*/true);
				auto [keep, px] = elements<T>(array);
				std::vector<T> copy(px.begin(), px.end());
				ch.set_chunk(std::span<T>(copy), index);
				return 0;
			});
		}
		py::array get_decompressed() const
		{
			return visit([]<typename T>(compressed::channel<T>& ch) {
				// numpy owns the pixels from the start (np.empty): the engine's D2H copy is the only pass over them
				py::array out = pooled_array<T>({ static_cast<py::ssize_t>(ch.height()), static_cast<py::ssize_t>(ch.width()) });
				ch.decompress_into(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(out.size())));
				return out;
			});
		}

		// the rectangle (x, y, width, height) as a (height, width) array: only the blocks it meets are decoded
		// (step_x, step_y > 1: every step_y-th row and every step_x-th element of it, a (ceil(height / step_y), ceil(width / step_x)) array;
		// only the blocks that hold a sampled element are decoded)
		py::array get_region(py::ssize_t x, py::ssize_t y, py::ssize_t width, py::ssize_t height, py::ssize_t step_x, py::ssize_t step_y) const
		{
			if (x < 0 || y < 0 || width < 0 || height < 0) throw py::value_error("region coordinates and sizes must be >= 0");
			check_steps(step_x, step_y);
			return visit([&]<typename T>(compressed::channel<T>& ch) {
				ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
				if (step_x == 1 && step_y == 1)
				{
					py::array out(np_dtype<T>(), std::vector<py::ssize_t>{ height, width });
					ch.get_region(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(width * height)), static_cast<size_t>(x),
						static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
					return out;
				}
				py::array out(np_dtype<T>(), std::vector<py::ssize_t>{ ceil_div(height, step_y), ceil_div(width, step_x) });
				ch.get_region(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(out.size())), static_cast<size_t>(x),
					static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height), static_cast<size_t>(step_x), static_cast<size_t>(step_y));
				return out;
			});
		}

		// N rectangles of one size at (xs[i], ys[i]) as an (N, h', w') array (pixels: 1 x 1 regions as an (N,) array): one engine call
		// that decodes every block once
		py::array get_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, py::ssize_t step_x, py::ssize_t step_y,
			bool pixels) const
		{
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			return visit([&]<typename T>(compressed::channel<T>& ch) {
				ch.check_regions(regions);
				py::array out(np_dtype<T>(), regions_shape(regions.size(), std::nullopt, width, height, step_x, step_y, pixels));
				if (out.size() > 0) ch.get_regions(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(out.size())), regions);
				return out;
			});
		}

		// the (height, width) array over the rectangle at (x, y): only the blocks it meets are decoded and re-encoded
		// array: (h', w'), written over every step_y-th row and step_x-th element from (x, y)
		void set_region(py::ssize_t x, py::ssize_t y, const py::array& array, py::ssize_t step_x, py::ssize_t step_y)
		{
			if (x < 0 || y < 0) throw py::value_error("region coordinates must be >= 0");
			check_steps(step_x, step_y);
			visit([&]<typename T>(compressed::channel<T>& ch) {
				const auto [hs, ws] = region_shape<T>(array);
				const size_t w = covered(static_cast<py::ssize_t>(ws), step_x), h = covered(static_cast<py::ssize_t>(hs), step_y);
				ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				auto [keep, px] = elements<T>(array);
				if (step_x == 1 && step_y == 1) ch.set_region(px, static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				else ch.set_region(px, static_cast<size_t>(x), static_cast<size_t>(y), w, h, static_cast<size_t>(step_x), static_cast<size_t>(step_y));
				return 0;
			});
		}
		// arrays: (N, h', w') (pixels: (N,)), region k from (xs[k], ys[k]); later regions win
		void set_regions(const py::object& xs, const py::object& ys, const py::array& arrays, py::ssize_t step_x, py::ssize_t step_y, bool pixels)
		{
			const std::string what = pixels ? "set_pixels" : "set_regions";
			check_steps(step_x, step_y);
			if (arrays.ndim() != (pixels ? 1 : 3)) throw py::value_error(what + (pixels ? ": values must have the shape (N,)" : ": arrays must have the shape (N, height, width)"));
			const auto regions = region_list(xs, ys, pixels ? 1 : static_cast<py::ssize_t>(covered(arrays.shape(2), step_x)),
				pixels ? 1 : static_cast<py::ssize_t>(covered(arrays.shape(1), step_y)), step_x, step_y);
			if (regions.size() != static_cast<size_t>(arrays.shape(0)))
				throw py::value_error(what + ": got " + std::to_string(arrays.shape(0)) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(compressed::channel<T>& ch) {
				if (!arrays.dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
				ch.check_regions(regions);
				auto [keep, px] = elements<T>(arrays);
				ch.set_regions(regions, px);
				return 0;
			});
		}
		// set_region / set_regions through mattes (mask: (h', w') / (N, h', w') numpy, bool or uint8): np.copyto(view, array, where=mask)
		void set_regions_masked(const py::object& xs, const py::object& ys, const py::array& arrays, py::ssize_t step_x, py::ssize_t step_y,
			const py::object& masks, bool single)
		{
			const char* what = single ? "set_region" : "set_regions";
			check_steps(step_x, step_y);
			const py::ssize_t nd = single ? 2 : 3;
			if (arrays.ndim() != nd) throw py::value_error(std::string(what) + (single ? ": the array must have the shape (height, width)" : ": arrays must have the shape (N, height, width)"));
			const auto regions = region_list(xs, ys, static_cast<py::ssize_t>(covered(arrays.shape(nd - 1), step_x)),
				static_cast<py::ssize_t>(covered(arrays.shape(nd - 2), step_y)), step_x, step_y);
			if (!single && regions.size() != static_cast<size_t>(arrays.shape(0)))
				throw py::value_error(std::string(what) + ": got " + std::to_string(arrays.shape(0)) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(compressed::channel<T>& ch) {
				if (!arrays.dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
				auto [mkeep, m] = host_mask(masks, std::vector<py::ssize_t>(arrays.shape(), arrays.shape() + arrays.ndim()), what);
				ch.check_regions(regions);
				auto [keep, px] = elements<T>(arrays);
				ch.set_regions(regions, px, m);
				return 0;
			});
		}
		// fill_region / fill_regions: value a number (fill_regions: or N numbers), masks (h', w') / (N, h', w') or None
		void fill_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, const py::object& value,
			py::ssize_t step_x, py::ssize_t step_y, const py::object& masks, bool single)
		{
			const char* what = single ? "fill_region" : "fill_regions";
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			visit([&]<typename T>(compressed::channel<T>& ch) {
				const std::vector<T> values = fill_values<T>(value, single ? 0 : regions.size(), what);
				std::vector<py::ssize_t> shape{ ceil_div(height, step_y), ceil_div(width, step_x) };
				if (!single) shape.insert(shape.begin(), static_cast<py::ssize_t>(regions.size()));
				ch.check_regions(regions);
				if (masks.is_none()) { ch.fill_regions(regions, values); return 0; }
				auto [mkeep, m] = host_mask(masks, shape, what);
				ch.fill_regions(regions, values, m);
				return 0;
			});
		}
		// a[key] = value for the keys of __getitem__: anything numpy.broadcast_to(numpy.asarray(value), selection shape) accepts;
		// scalars and sequences are converted to the channel's dtype, an ARRAY of another dtype is refused
		void setitem(const py::object& key, const py::object& value)
		{
			visit([&]<typename T>(compressed::channel<T>& ch) {
				const region_pick p = pick_region(key, static_cast<py::ssize_t>(ch.height()), static_cast<py::ssize_t>(ch.width()));
				const py::module_ np = py::module_::import("numpy");
				py::object a = value;
				if (py::isinstance<py::array>(value))
				{
					if (!py::array(value).dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
				}
				else a = np.attr("asarray")(value, py::arg("dtype") = np_dtype<T>());
				const py::array b = np.attr("ascontiguousarray")(np.attr("broadcast_to")(a, py::cast(p.shape)));
				if (p.w > 0 && p.h > 0)
					ch.set_region(std::span<const T>(static_cast<const T*>(b.data()), static_cast<size_t>(b.size())), static_cast<size_t>(p.x),
						static_cast<size_t>(p.y), static_cast<size_t>(p.w), static_cast<size_t>(p.h), static_cast<size_t>(p.sx), static_cast<size_t>(p.sy));
				return 0;
			});
		}

		template <typename T> static std::pair<size_t, size_t> region_shape(const py::array& a)
		{
			if (!a.dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
			if (a.ndim() != 2) throw py::value_error("region arrays must be two-dimensional (height, width), got " + std::to_string(a.ndim()) + " dimensions");
			return { static_cast<size_t>(a.shape(0)), static_cast<size_t>(a.shape(1)) };
		}

		template <typename T> static void check_chunk_array(const py::array& a, size_t elems, bool exact)
		{
			if (!a.dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
			if (a.ndim() != 1) throw py::value_error("chunk arrays must be one-dimensional, got " + std::to_string(a.ndim()) + " dimensions");
			const size_t n = static_cast<size_t>(a.size());
			if (exact ? n != elems : n < elems)
				throw py::value_error("chunk array has " + std::to_string(n) + " elements, expected " + std::to_string(elems));
		}
	};

	// ---- Image ------------------------------------------------------------------------------------------------
	template <typename T> using img_ptr = std::shared_ptr<compressed::image<T>>;
	using any_image = std::variant<img_ptr<compressed::half>, img_ptr<float>, img_ptr<double>, img_ptr<uint8_t>, img_ptr<int8_t>,
		img_ptr<uint16_t>, img_ptr<int16_t>, img_ptr<uint32_t>, img_ptr<int32_t>>;

	struct Image
	{
		any_image impl;
		py::dict metadata;

		template <typename F> auto visit(F&& f) const { return std::visit([&](auto& p) { return f(p); }, impl); }

		explicit Image(any_image adopted) : impl(std::move(adopted)) {}          // (DeviceImage.to_image)
		Image(const py::object& dtype, const std::vector<py::array>& channels, size_t width, size_t height, std::vector<std::string> names,
			codec c, size_t level, size_t block, size_t chunk, std::optional<int> mantissa)
		{
			impl = dispatch(as_dtype(dtype), [&]<typename T>() -> any_image {
				compressed::blosc2::ensure_mantissa_bits<T>(mantissa);
				std::vector<py::array> keep;
				std::vector<std::span<const T>> spans;
				for (const auto& a : channels)
				{
					if (!a.dtype().is(np_dtype<T>())) throw py::value_error("channel dtype does not match the image dtype");
					auto [k, px] = elements<T>(a);
					keep.push_back(k);
					spans.push_back(px);
				}
				try { return std::make_shared<compressed::image<T>>(spans, width, height, std::move(names), c, level, block, chunk, mantissa); }
				catch (const std::runtime_error& e) { throw py::value_error(e.what()); }
			});
		}

		void add_channel(const py::array& data, size_t width, size_t height, std::optional<std::string> name, codec c, size_t level, size_t block, size_t chunk, std::optional<int> mantissa)
		{
			visit([&]<typename T>(const img_ptr<T>& img) {
				compressed::blosc2::ensure_mantissa_bits<T>(mantissa);
				if (!data.dtype().is(np_dtype<T>())) throw py::value_error("channel dtype does not match the image dtype");
				if (data.ndim() == 2 && (static_cast<size_t>(data.shape(0)) != height || static_cast<size_t>(data.shape(1)) != width))
					throw py::value_error("array shape does not match (height, width)");
				auto [keep, px] = elements<T>(data);
				if (px.size() != width * height) throw py::value_error("array size does not match width * height");
				compressed::channel<T> ch(px, width, height, c, static_cast<uint8_t>(std::min<size_t>(level, 255)), block, chunk, mantissa);
				img->add_channel(std::move(ch), std::move(name));
				return 0;
			});
		}
		void remove_channel(const std::variant<std::string, size_t>& key)
		{
			visit([&](auto& img) {
				if (std::holds_alternative<size_t>(key)) img->remove_channel(std::get<size_t>(key));
				else img->remove_channel(std::string_view(std::get<std::string>(key)));
				return 0;
			});
		}
		Channel channel(const std::variant<std::string, size_t>& key) const
		{
			return visit([&]<typename T>(const img_ptr<T>& img) {
				auto& ch = std::holds_alternative<size_t>(key) ? img->channel(std::get<size_t>(key)) : img->channel(std::string_view(std::get<std::string>(key)));
				return Channel{ chan_ptr<T>(img, &ch) };          // aliases the image: keeps it alive
			});
		}
		std::vector<Channel> channels() const
		{
			std::vector<Channel> out;
			const size_t n = visit([](auto& img) { return img->num_channels(); });
			for (size_t i = 0; i < n; ++i) out.push_back(channel(i));
			return out;
		}
		// the rectangle of every channel, one engine call: a list of (height, width) arrays
		py::list get_region(py::ssize_t x, py::ssize_t y, py::ssize_t width, py::ssize_t height, py::ssize_t step_x, py::ssize_t step_y) const
		{
			if (x < 0 || y < 0 || width < 0 || height < 0) throw py::value_error("region coordinates and sizes must be >= 0");
			check_steps(step_x, step_y);
			if (step_x > 1 || step_y > 1)
				return visit([&]<typename T>(const img_ptr<T>& img) {
					compressed::blosc2::batch::strided_window_job job;
					py::list out;
					for (const auto& ch : img->channels())
					{
						ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
						py::array a(np_dtype<T>(), std::vector<py::ssize_t>{ ceil_div(height, step_y), ceil_div(width, step_x) });
						ch.plan_region(static_cast<T*>(a.mutable_data()), static_cast<size_t>(a.shape(1)), static_cast<size_t>(x), static_cast<size_t>(y),
							static_cast<size_t>(width), static_cast<size_t>(height), static_cast<size_t>(step_x), static_cast<size_t>(step_y), job);
						out.append(a);
					}
					compressed::blosc2::batch::decompress_windows(job);
					return out;
				});
			return visit([&]<typename T>(const img_ptr<T>& img) {
				compressed::blosc2::batch::window_job job;
				std::vector<py::array> arrays;
				for (const auto& ch : img->channels())
				{
					ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
					py::array a(np_dtype<T>(), std::vector<py::ssize_t>{ height, width });
					ch.plan_region(static_cast<T*>(a.mutable_data()), static_cast<size_t>(width), static_cast<size_t>(x), static_cast<size_t>(y),
						static_cast<size_t>(width), static_cast<size_t>(height), job);
					arrays.push_back(a);
				}
				compressed::blosc2::batch::decompress_windows(job);
				py::list out;
				for (auto& a : arrays) out.append(a);
				return out;
			});
		}
		// N rectangles of every channel as an (N, C, h', w') array (pixels: an (N, C) array): one engine call
		py::array get_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, py::ssize_t step_x, py::ssize_t step_y,
			bool pixels) const
		{
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			return visit([&]<typename T>(const img_ptr<T>& img) {
				img->check_regions(regions);
				py::array out(np_dtype<T>(), regions_shape(regions.size(), img->num_channels(), width, height, step_x, step_y, pixels));
				if (out.size() > 0) img->get_regions(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(out.size())), regions);
				return out;
			});
		}
		// one (height, width) array per channel over the rectangle at (x, y): one engine call
		void set_region(py::ssize_t x, py::ssize_t y, const std::vector<py::array>& arrays, py::ssize_t step_x, py::ssize_t step_y)
		{
			if (x < 0 || y < 0) throw py::value_error("region coordinates must be >= 0");
			check_steps(step_x, step_y);
			visit([&]<typename T>(const img_ptr<T>& img) {
				if (arrays.size() != img->num_channels())
					throw py::value_error("got " + std::to_string(arrays.size()) + " arrays for " + std::to_string(img->num_channels()) + " channels");
				std::vector<py::array> keep;
				std::vector<std::span<const T>> spans;
				size_t h = 0, w = 0;
				for (size_t i = 0; i < arrays.size(); ++i)
				{
					const auto [hi, wi] = Channel::region_shape<T>(arrays[i]);
					if (i > 0 && (hi != h || wi != w)) throw py::value_error("region arrays must all have the same shape");
					h = hi; w = wi;
					auto [k, px] = elements<T>(arrays[i]);
					keep.push_back(k);
					spans.push_back(px);
				}
				const size_t cw = covered(static_cast<py::ssize_t>(w), step_x), chh = covered(static_cast<py::ssize_t>(h), step_y);
				for (const auto& ch : img->channels()) ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), cw, chh);
				if (step_x == 1 && step_y == 1) img->set_region(spans, static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				else img->set_region(spans, static_cast<size_t>(x), static_cast<size_t>(y), cw, chh, static_cast<size_t>(step_x), static_cast<size_t>(step_y));
				return 0;
			});
		}
		// arrays: (N, C, h', w') (pixels: (N, C)), region k from (xs[k], ys[k]) of every channel; later regions win
		void set_regions(const py::object& xs, const py::object& ys, const py::array& arrays, py::ssize_t step_x, py::ssize_t step_y, bool pixels)
		{
			const std::string what = pixels ? "set_pixels" : "set_regions";
			check_steps(step_x, step_y);
			if (arrays.ndim() != (pixels ? 2 : 4)) throw py::value_error(what + (pixels ? ": values must have the shape (N, channels)" : ": arrays must have the shape (N, channels, height, width)"));
			const auto regions = region_list(xs, ys, pixels ? 1 : static_cast<py::ssize_t>(covered(arrays.shape(3), step_x)),
				pixels ? 1 : static_cast<py::ssize_t>(covered(arrays.shape(2), step_y)), step_x, step_y);
			if (regions.size() != static_cast<size_t>(arrays.shape(0)))
				throw py::value_error(what + ": got " + std::to_string(arrays.shape(0)) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(const img_ptr<T>& img) {
				if (!arrays.dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the image dtype");
				if (static_cast<size_t>(arrays.shape(1)) != img->num_channels()) throw py::value_error(what + ": the arrays' channel count does not match the image");
				img->check_regions(regions);
				auto [keep, px] = elements<T>(arrays);
				img->set_regions(regions, px);
				return 0;
			});
		}
		// set_region / set_regions of every channel through ONE shared matte: arrays a list of C (h', w') arrays (set_region) or
		// (N, C, h', w') (set_regions); mask (h', w') / (N, h', w'), numpy bool or uint8
		void set_regions_masked(const py::object& xs, const py::object& ys, const py::object& arrays_in, py::ssize_t step_x, py::ssize_t step_y,
			const py::object& masks, bool single)
		{
			const char* what = single ? "set_region" : "set_regions";
			check_steps(step_x, step_y);
			py::module_ np = py::module_::import("numpy");
			py::array arrays = single ? py::array(np.attr("stack")(arrays_in)) : py::array(np.attr("asarray")(arrays_in));   // (C, h', w') / (N, C, h', w')
			const py::ssize_t nd = single ? 3 : 4;
			if (arrays.ndim() != nd) throw py::value_error(std::string(what) + (single ? ": one (height, width) array a channel" : ": arrays must have the shape (N, channels, height, width)"));
			const auto regions = region_list(xs, ys, static_cast<py::ssize_t>(covered(arrays.shape(nd - 1), step_x)),
				static_cast<py::ssize_t>(covered(arrays.shape(nd - 2), step_y)), step_x, step_y);
			if (!single && regions.size() != static_cast<size_t>(arrays.shape(0)))
				throw py::value_error(std::string(what) + ": got " + std::to_string(arrays.shape(0)) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(const img_ptr<T>& img) {
				if (!arrays.dtype().is(np_dtype<T>())) throw py::value_error("array dtype does not match the image dtype");
				if (static_cast<size_t>(arrays.shape(nd - 3)) != img->num_channels()) throw py::value_error(std::string(what) + ": the arrays' channel count does not match the image");
				std::vector<py::ssize_t> mshape{ arrays.shape(nd - 2), arrays.shape(nd - 1) };
				if (!single) mshape.insert(mshape.begin(), arrays.shape(0));
				auto [mkeep, m] = host_mask(masks, mshape, what);
				img->check_regions(regions);
				auto [keep, px] = elements<T>(arrays);
				img->set_regions(regions, px, m);
				return 0;
			});
		}
		// fill_region / fill_regions of every channel: value a number or C numbers, masks shared by the channels
		void fill_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, const py::object& value,
			py::ssize_t step_x, py::ssize_t step_y, const py::object& masks, bool single)
		{
			const char* what = single ? "fill_region" : "fill_regions";
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			visit([&]<typename T>(const img_ptr<T>& img) {
				const std::vector<T> values = fill_values<T>(value, img->num_channels(), what);
				std::vector<py::ssize_t> shape{ ceil_div(height, step_y), ceil_div(width, step_x) };
				if (!single) shape.insert(shape.begin(), static_cast<py::ssize_t>(regions.size()));
				img->check_regions(regions);
				if (masks.is_none()) { img->fill_regions(regions, values); return 0; }
				auto [mkeep, m] = host_mask(masks, shape, what);
				img->fill_regions(regions, values, m);
				return 0;
			});
		}
		py::array get_decompressed() const
		{
			return visit([]<typename T>(const img_ptr<T>& img) {
				py::array out = pooled_array<T>({ static_cast<py::ssize_t>(img->num_channels()),
					static_cast<py::ssize_t>(img->height()), static_cast<py::ssize_t>(img->width()) });
				img->decompress_into(std::span<T>(static_cast<T*>(out.mutable_data()), static_cast<size_t>(out.size())));
				return out;
			});
		}
	};

	// ---- device-resident objects ----------------------------------------------------------------------------
	// Inputs and out= arguments are any object with __cuda_array_interface__ (torch ROCm tensors have it): dtype from `typestr`,
	// C-contiguous only.  Everything about an argument is checked before the engine is touched; the address itself is checked by
	// the C++ layer (cimg_device_range_check) before a kernel sees it.
	struct device_view
	{
		void* ptr = nullptr;
		std::vector<py::ssize_t> shape;
		py::dtype dt;
		bool readonly = false;
		size_t count() const { size_t n = 1; for (auto d : shape) n *= static_cast<size_t>(d); return n; }
	};
	device_view view_of(const py::object& o, const char* what)
	{
		if (py::isinstance<py::array>(o))
			throw py::type_error(std::string(what) + ": a numpy array is host memory; pass an object with __cuda_array_interface__ (a torch tensor on the GPU)");
		if (!py::hasattr(o, "__cuda_array_interface__"))
			throw py::type_error(std::string(what) + ": expected an object with __cuda_array_interface__");
		py::dict d = o.attr("__cuda_array_interface__");
		device_view v;
		for (auto n : d["shape"].cast<py::tuple>()) v.shape.push_back(n.cast<py::ssize_t>());
		v.dt = py::dtype::from_args(d["typestr"]);
		py::tuple data = d["data"];
		v.ptr = reinterpret_cast<void*>(data[0].cast<uintptr_t>());
		v.readonly = data[1].cast<bool>();
		if (d.contains("strides") && !d["strides"].is_none())
		{
			py::ssize_t dense = v.dt.itemsize();
			py::tuple st = d["strides"];
			if (st.size() != v.shape.size()) throw py::value_error(std::string(what) + ": strides and shape disagree");
			for (size_t k = v.shape.size(); k-- > 0;)
			{
				if (v.shape[k] != 1 && st[k].cast<py::ssize_t>() != dense) throw py::value_error(std::string(what) + ": the array is not C-contiguous");
				dense *= v.shape[k];
			}
		}
		if (v.count() > 0 && !v.ptr) throw py::value_error(std::string(what) + ": null device address");
		return v;
	}
	void wait_for(const std::optional<uintptr_t>& stream)
	{
		if (stream) compressed::device_channel<uint8_t>::wait_stream(reinterpret_cast<void*>(*stream));
	}

	// Results with out=None: device memory from cimg_device_malloc, exposed through __cuda_array_interface__ (version 2), so that
	// torch.as_tensor(r, device="cuda") wraps it without a copy (the tensor keeps this object alive).
	struct DeviceArray
	{
		std::shared_ptr<void> mem;
		std::vector<py::ssize_t> shape;
		py::dtype dt;
		size_t nbytes = 0;

		DeviceArray(std::vector<py::ssize_t> shape_, py::dtype dt_) : shape(std::move(shape_)), dt(std::move(dt_))
		{
			nbytes = static_cast<size_t>(dt.itemsize());
			for (auto d : shape) nbytes *= static_cast<size_t>(d);
			cimg_engine* e = compressed::blosc2::batch::engine();
			void* p = cimg_device_malloc(e, std::max<size_t>(nbytes, 1));        // (an empty selection still has an address)
			if (!p) throw std::runtime_error(std::string("Unable to allocate device memory: ") + cimg_last_error(e));
			mem = std::shared_ptr<void>(p, [e](void* q) { cimg_device_free(e, q); });
		}
		py::dict interface() const
		{
			py::dict d;
			d["version"] = 2;
			d["shape"] = py::tuple(py::cast(shape));
			d["typestr"] = dt.attr("str");
			d["data"] = py::make_tuple(reinterpret_cast<uintptr_t>(mem.get()), false);
			d["strides"] = py::none();
			return d;
		}
		py::array copy_to_host() const
		{
			py::array out(dt, shape);
			cimg_engine* e = compressed::blosc2::batch::engine();
			if (nbytes && cimg_memcpy_d2h(e, out.mutable_data(), mem.get(), nbytes) < 0) throw std::runtime_error(cimg_last_error(e));
			return out;
		}
	};

	// where a result goes: the caller's `out` (checked: dtype, shape, writable, contiguous) or a new DeviceArray
	template <typename T> std::pair<T*, py::object> result_target(const py::object& out, const std::vector<py::ssize_t>& shape, const char* what)
	{
		if (out.is_none())
		{
			DeviceArray a(shape, np_dtype<T>());
			T* p = static_cast<T*>(a.mem.get());
			return { p, py::cast(std::move(a)) };
		}
		const device_view v = view_of(out, what);
		if (!v.dt.is(np_dtype<T>())) throw py::type_error(std::string(what) + ": out has dtype " + std::string(py::str(v.dt)) + ", expected " + dtype_code<T>());
		if (v.shape != shape) throw py::value_error(std::string(what) + ": out has the wrong shape");
		if (v.readonly) throw py::value_error(std::string(what) + ": out is read-only");
		return { static_cast<T*>(v.ptr), out };
	}
	// ---- typed reads (device_channel.h / device_image.h: get_region<U>, get_regions<U>) ----
	// scale= / offset=: a number, or a sequence of one value per channel
	inline std::vector<float> float_list(const py::object& o, size_t channels, const char* name)
	{
		std::vector<float> v;
		if (py::hasattr(o, "__len__")) for (auto h : o) v.push_back(static_cast<float>(h.cast<double>()));
		else v.push_back(static_cast<float>(o.cast<double>()));
		if (v.size() != 1 && v.size() != channels)
			throw py::value_error(std::string(name) + ": expected a number or one value per channel (" + std::to_string(channels) + "), got " + std::to_string(v.size()));
		return v;
	}
	// without dtype= nothing is converted: scale and offset must be left at 1 and 0
	inline void require_plain(const std::vector<float>& scales, const std::vector<float>& offsets, const char* what)
	{
		for (float s : scales) if (s != 1.0f) throw py::value_error(std::string(what) + ": scale needs dtype= (float32, float16)");
		for (float o : offsets) if (o != 0.0f) throw py::value_error(std::string(what) + ": offset needs dtype= (float32, float16)");
	}
	// f.template operator()<U>() for the result type dtype= names: the stored type T, float or half
	template <typename T, typename F> py::object typed_dispatch(const py::object& dtype, F&& f, const char* what)
	{
		const py::dtype dt = as_dtype(dtype);
		if (dt.is(np_dtype<T>())) return f.template operator()<T>();
		if (dt.is(np_dtype<float>())) return f.template operator()<float>();
		if (dt.is(np_dtype<compressed::half>())) return f.template operator()<compressed::half>();
		throw py::value_error(std::string(what) + ": dtype must be float32, float16 or the stored dtype, got " + std::string(py::str(dt)));
	}

	// f.template operator()<U>() for the source type dtype= names -- the stored type T, float or half; the array must hold exactly that
	template <typename T, typename F> void typed_source_dispatch(const py::object& dtype, const py::dtype& have, F&& f, const char* what)
	{
		const py::dtype dt = as_dtype(dtype);
		const bool stored = dt.is(np_dtype<T>()), f32 = dt.is(np_dtype<float>()), f16 = dt.is(np_dtype<compressed::half>());
		if (!stored && !f32 && !f16)
			throw py::value_error(std::string(what) + ": dtype must be float32, float16 or the stored dtype, got " + std::string(py::str(dt)));
		if (!have.is(dt))
			throw py::type_error(std::string(what) + ": the array has dtype " + std::string(py::str(have)) + ", dtype= says " + std::string(py::str(dt)));
		if (stored) f.template operator()<T>();
		else if (f32) f.template operator()<float>();
		else f.template operator()<compressed::half>();
	}

	inline void check_region_args(py::ssize_t x, py::ssize_t y, py::ssize_t w, py::ssize_t h)
	{
		if (x < 0 || y < 0 || w < 0 || h < 0) throw py::value_error("region coordinates and sizes must be >= 0");
	}

	// mask= / masks= of the device classes: bool or uint8 in device memory, of exactly `shape`
	inline const uint8_t* device_mask(const py::object& mask, const std::vector<py::ssize_t>& shape, const char* what)
	{
		const device_view m = view_of(mask, what);
		if (!m.dt.is(py::dtype("uint8")) && !m.dt.is(py::dtype("bool")))
			throw py::value_error(std::string(what) + ": a mask has dtype bool or uint8, got " + std::string(py::str(m.dt)));
		if (m.shape != shape) throw py::value_error(std::string(what) + ": the mask's shape does not match the written elements' shape");
		return static_cast<const uint8_t*>(m.ptr);
	}
	template <typename T> using dchan_ptr = std::shared_ptr<compressed::device_channel<T>>;
	using any_dchannel = std::variant<dchan_ptr<compressed::half>, dchan_ptr<float>, dchan_ptr<double>, dchan_ptr<uint8_t>, dchan_ptr<int8_t>,
		dchan_ptr<uint16_t>, dchan_ptr<int16_t>, dchan_ptr<uint32_t>, dchan_ptr<int32_t>>;

	struct DeviceChannel
	{
		any_dchannel impl;
		template <typename F> auto visit(F&& f) const { return std::visit([&](auto& p) { return f(*p); }, impl); }

		static DeviceChannel from_array(const py::object& data, size_t width, size_t height, codec c, size_t level, size_t block, size_t chunk,
			std::optional<uintptr_t> stream, std::optional<int> mantissa)
		{
			const device_view v = view_of(data, "DeviceChannel");
			return dispatch(v.dt, [&]<typename T>() {
				compressed::blosc2::ensure_mantissa_bits<T>(mantissa);
				if (v.count() != width * height)
					throw py::value_error("Channel data has " + std::to_string(v.count()) + " elements, expected width * height = " + std::to_string(width * height));
				wait_for(stream);
				return DeviceChannel{ std::make_shared<compressed::device_channel<T>>(static_cast<const T*>(v.ptr), width, height, c,
					static_cast<uint8_t>(std::min<size_t>(level, 255)), block, chunk, mantissa) };
			});
		}
		std::optional<int> mantissa_bits() const { return visit([](auto& c) { return c.mantissa_bits(); }); }
		// blank channels: special-value chunks written on the host, 64 bytes of device memory a chunk (device_channel.h: full)
		static DeviceChannel full(const py::object& dtype, const py::object& fill, size_t width, size_t height, codec c, size_t level, size_t block, size_t chunk,
			std::optional<int> mantissa)
		{
			return dispatch(as_dtype(dtype), [&]<typename T>() {
				return DeviceChannel{ std::make_shared<compressed::device_channel<T>>(compressed::device_channel<T>::full(from_scalar<T>(fill), width, height, c,
					static_cast<uint8_t>(std::min<size_t>(level, 255)), block, chunk, mantissa)) };
			});
		}
		static DeviceChannel full_like(const DeviceChannel& other, const py::object& fill)
		{
			return other.visit([&]<typename T>(compressed::device_channel<T>& ch) {
				return DeviceChannel{ std::make_shared<compressed::device_channel<T>>(compressed::device_channel<T>::full_like(ch, from_scalar<T>(fill))) };
			});
		}
		static DeviceChannel from_channel(const Channel& host)
		{
			return host.visit([]<typename T>(compressed::channel<T>& ch) {
				return DeviceChannel{ std::make_shared<compressed::device_channel<T>>(compressed::device_channel<T>::from_channel(ch)) };
			});
		}
		Channel to_channel() const
		{
			return visit([]<typename T>(compressed::device_channel<T>& ch) { return Channel{ std::make_shared<compressed::channel<T>>(ch.to_channel()) }; });
		}
		py::object get_decompressed(const py::object& out, std::optional<uintptr_t> stream) const
		{
			return visit([&]<typename T>(compressed::device_channel<T>& ch) {
				auto [p, ret] = result_target<T>(out, { static_cast<py::ssize_t>(ch.height()), static_cast<py::ssize_t>(ch.width()) }, "get_decompressed");
				wait_for(stream);
				ch.decompress_into(p);
				return ret;
			});
		}
		py::object get_region(py::ssize_t x, py::ssize_t y, py::ssize_t width, py::ssize_t height, const py::object& out, std::optional<uintptr_t> stream,
			py::ssize_t step_x, py::ssize_t step_y, const py::object& dtype, const py::object& scale, const py::object& offset) const
		{
			check_region_args(x, y, width, height);
			check_steps(step_x, step_y);
			const std::vector<float> sc = float_list(scale, 1, "scale"), of = float_list(offset, 1, "offset");
			if (dtype.is_none()) require_plain(sc, of, "get_region");
			return visit([&]<typename T>(compressed::device_channel<T>& ch) -> py::object {
				ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
				if (!dtype.is_none())
					return typed_dispatch<T>(dtype, [&]<typename U>() -> py::object {
						auto [p, ret] = result_target<U>(out, { ceil_div(height, step_y), ceil_div(width, step_x) }, "get_region");
						wait_for(stream);
						ch.get_region(p, static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height),
							static_cast<size_t>(step_x), static_cast<size_t>(step_y), sc[0], of[0]);
						return ret;
					}, "get_region");
				auto [p, ret] = result_target<T>(out, { ceil_div(height, step_y), ceil_div(width, step_x) }, "get_region");
				wait_for(stream);
				if (step_x == 1 && step_y == 1)
					ch.get_region(p, static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
				else
					ch.get_region(p, static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height),
						static_cast<size_t>(step_x), static_cast<size_t>(step_y));
				return ret;
			});
		}
		// Channel.get_regions / get_pixels into device memory: `out` or a new DeviceArray
		py::object get_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, const py::object& out,
			std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y, bool pixels, const py::object& dtype = py::none(),
			const py::object& scale = py::float_(1.0), const py::object& offset = py::float_(0.0)) const
		{
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			const char* what = pixels ? "get_pixels" : "get_regions";
			const std::vector<float> sc = float_list(scale, 1, "scale"), of = float_list(offset, 1, "offset");
			if (dtype.is_none()) require_plain(sc, of, what);
			return visit([&]<typename T>(compressed::device_channel<T>& ch) -> py::object {
				ch.check_regions(regions);
				if (!dtype.is_none())
					return typed_dispatch<T>(dtype, [&]<typename U>() -> py::object {
						auto [p, ret] = result_target<U>(out, regions_shape(regions.size(), std::nullopt, width, height, step_x, step_y, pixels), what);
						wait_for(stream);
						ch.get_regions(p, std::span<const compressed::region>(regions), sc[0], of[0]);
						return ret;
					}, what);
				auto [p, ret] = result_target<T>(out, regions_shape(regions.size(), std::nullopt, width, height, step_x, step_y, pixels),
					pixels ? "get_pixels" : "get_regions");
				wait_for(stream);
				ch.get_regions(p, regions);
				return ret;
			});
		}
		// a[key] as Channel.__getitem__ has it, into a new DeviceArray
		py::object getitem(const py::object& key) const
		{
			return visit([&]<typename T>(compressed::device_channel<T>& ch) {
				const region_pick p = pick_region(key, static_cast<py::ssize_t>(ch.height()), static_cast<py::ssize_t>(ch.width()));
				auto [d, ret] = result_target<T>(py::none(), p.shape, "__getitem__");
				if (p.w > 0 && p.h > 0)
					ch.get_region(d, static_cast<size_t>(p.x), static_cast<size_t>(p.y), static_cast<size_t>(p.w), static_cast<size_t>(p.h),
						static_cast<size_t>(p.sx), static_cast<size_t>(p.sy));
				return ret;
			});
		}
		// array: (h', w') in device memory, written over every step_y-th row and step_x-th element from (x, y)
		// (dtype=: the array holds float32, float16 or the stored type and every element is unscaled, rounded and stored in the patch launch)
		void set_region(py::ssize_t x, py::ssize_t y, const py::object& array, std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y,
			const py::object& dtype = py::none(), const py::object& scale = py::float_(1.0), const py::object& offset = py::float_(0.0),
			const py::object& mask = py::none())
		{
			if (x < 0 || y < 0) throw py::value_error("region coordinates must be >= 0");
			check_steps(step_x, step_y);
			const std::vector<float> sc = float_list(scale, 1, "scale"), of = float_list(offset, 1, "offset");
			if (dtype.is_none()) require_plain(sc, of, "set_region");
			if (!mask.is_none() && !dtype.is_none()) throw py::value_error("set_region: mask= cannot be combined with dtype= (masked typed writes are not built)");
			const device_view v = view_of(array, "set_region");
			visit([&]<typename T>(compressed::device_channel<T>& ch) {
				if (!mask.is_none())
				{
					if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
					if (v.shape.size() != 2) throw py::value_error("region arrays must be two-dimensional (height, width), got " + std::to_string(v.shape.size()) + " dimensions");
					const uint8_t* m = device_mask(mask, v.shape, "set_region");
					const size_t w = covered(v.shape[1], step_x), h = covered(v.shape[0], step_y);
					ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), w, h);
					wait_for(stream);
					ch.set_region(static_cast<const T*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h, static_cast<size_t>(step_x),
						static_cast<size_t>(step_y), m);
					return 0;
				}
				if (!dtype.is_none())
				{
					typed_source_dispatch<T>(dtype, v.dt, [&]<typename U>() {
						if (v.shape.size() != 2) throw py::value_error("region arrays must be two-dimensional (height, width), got " + std::to_string(v.shape.size()) + " dimensions");
						const size_t w = covered(v.shape[1], step_x), h = covered(v.shape[0], step_y);
						ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), w, h);
						wait_for(stream);
						ch.set_region(static_cast<const U*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h, static_cast<size_t>(step_x),
							static_cast<size_t>(step_y), sc[0], of[0]);
					}, "set_region");
					return 0;
				}
				if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
				if (v.shape.size() != 2) throw py::value_error("region arrays must be two-dimensional (height, width), got " + std::to_string(v.shape.size()) + " dimensions");
				const size_t w = covered(v.shape[1], step_x), h = covered(v.shape[0], step_y);
				ch.check_region(static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				wait_for(stream);
				if (step_x == 1 && step_y == 1)
					ch.set_region(static_cast<const T*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				else
					ch.set_region(static_cast<const T*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h, static_cast<size_t>(step_x),
						static_cast<size_t>(step_y));
				return 0;
			});
		}
		// arrays: (N, h', w') in device memory (pixels: (N,)), region k from (xs[k], ys[k]); later regions win
		void set_regions(const py::object& xs, const py::object& ys, const py::object& arrays, std::optional<uintptr_t> stream, py::ssize_t step_x,
			py::ssize_t step_y, bool pixels, const py::object& dtype = py::none(), const py::object& scale = py::float_(1.0),
			const py::object& offset = py::float_(0.0), const py::object& masks = py::none())
		{
			const char* what = pixels ? "set_pixels" : "set_regions";
			check_steps(step_x, step_y);
			const std::vector<float> sc = float_list(scale, 1, "scale"), of = float_list(offset, 1, "offset");
			if (dtype.is_none()) require_plain(sc, of, what);
			if (!masks.is_none() && !dtype.is_none()) throw py::value_error(std::string(what) + ": masks= cannot be combined with dtype= (masked typed writes are not built)");
			const device_view v = view_of(arrays, what);
			if (v.shape.size() != (pixels ? 1u : 3u)) throw py::value_error(std::string(what) + (pixels ? ": values must have the shape (N,)" : ": arrays must have the shape (N, height, width)"));
			const auto regions = region_list(xs, ys, pixels ? 1 : static_cast<py::ssize_t>(covered(v.shape[2], step_x)),
				pixels ? 1 : static_cast<py::ssize_t>(covered(v.shape[1], step_y)), step_x, step_y);
			if (regions.size() != static_cast<size_t>(v.shape[0]))
				throw py::value_error(std::string(what) + ": got " + std::to_string(v.shape[0]) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(compressed::device_channel<T>& ch) {
				if (!dtype.is_none())
				{
					typed_source_dispatch<T>(dtype, v.dt, [&]<typename U>() {
						ch.check_regions(regions);
						wait_for(stream);
						ch.set_regions(std::span<const compressed::region>(regions), static_cast<const U*>(v.ptr), sc[0], of[0]);
					}, what);
					return 0;
				}
				if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
				const uint8_t* m = masks.is_none() ? nullptr : device_mask(masks, v.shape, what);
				ch.check_regions(regions);
				if (regions.empty() || v.count() == 0) return 0;
				wait_for(stream);
				if (m) ch.set_regions(regions, static_cast<const T*>(v.ptr), m);
				else ch.set_regions(regions, static_cast<const T*>(v.ptr));
				return 0;
			});
		}
		// paint every step_y-th row and step_x-th element of the rectangle with one value (mask: (h', w') bool / uint8 in device memory,
		// paint only where it is not 0): no source array exists anywhere
		void fill_region(py::ssize_t x, py::ssize_t y, py::ssize_t width, py::ssize_t height, const py::object& value, std::optional<uintptr_t> stream,
			py::ssize_t step_x, py::ssize_t step_y, const py::object& mask)
		{
			fill_regions(py::make_tuple(x), py::make_tuple(y), width, height, value, stream, step_x, step_y, mask, true);
		}
		// N rectangles of one size painted in one engine call: value a number or N numbers, masks (N, h', w')
		void fill_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, const py::object& value,
			std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y, const py::object& masks, bool single = false)
		{
			const char* what = single ? "fill_region" : "fill_regions";
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			visit([&]<typename T>(compressed::device_channel<T>& ch) {
				const std::vector<T> values = fill_values<T>(value, single ? 0 : regions.size(), what);
				std::vector<py::ssize_t> shape{ ceil_div(height, step_y), ceil_div(width, step_x) };
				if (!single) shape.insert(shape.begin(), static_cast<py::ssize_t>(regions.size()));
				const uint8_t* m = masks.is_none() ? nullptr : device_mask(masks, shape, what);
				ch.check_regions(regions);
				if (regions.empty() || width == 0 || height == 0) return 0;
				wait_for(stream);
				if (m) ch.fill_regions(std::span<const compressed::region>(regions), std::span<const T>(values), m);
				else ch.fill_regions(std::span<const compressed::region>(regions), std::span<const T>(values));
				return 0;
			});
		}
		// a[key] = value for the keys of __getitem__: value is a device array of exactly the selection's shape and dtype
		void setitem(const py::object& key, const py::object& value)
		{
			visit([&]<typename T>(compressed::device_channel<T>& ch) {
				const region_pick p = pick_region(key, static_cast<py::ssize_t>(ch.height()), static_cast<py::ssize_t>(ch.width()));
				const device_view v = view_of(value, "__setitem__");
				if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the channel dtype");
				if (v.shape != p.shape) throw py::value_error("__setitem__: the value's shape does not match the selection's shape");
				if (p.w > 0 && p.h > 0)
					ch.set_region(static_cast<const T*>(v.ptr), static_cast<size_t>(p.x), static_cast<size_t>(p.y), static_cast<size_t>(p.w),
						static_cast<size_t>(p.h), static_cast<size_t>(p.sx), static_cast<size_t>(p.sy));
				return 0;
			});
		}
	};

	template <typename T> using dimg_ptr = std::shared_ptr<compressed::device_image<T>>;
	using any_dimage = std::variant<dimg_ptr<compressed::half>, dimg_ptr<float>, dimg_ptr<double>, dimg_ptr<uint8_t>, dimg_ptr<int8_t>,
		dimg_ptr<uint16_t>, dimg_ptr<int16_t>, dimg_ptr<uint32_t>, dimg_ptr<int32_t>>;

	struct DeviceImage
	{
		any_dimage impl;
		template <typename F> auto visit(F&& f) const { return std::visit([&](auto& p) { return f(p); }, impl); }

		// channels: a list of (H, W) device arrays or one (C, H, W) device array
		static DeviceImage from_arrays(const py::object& dtype, const py::object& channels, size_t width, size_t height, std::vector<std::string> names,
			codec c, size_t level, size_t block, size_t chunk, std::optional<uintptr_t> stream, std::optional<int> mantissa)
		{
			const py::dtype dt = as_dtype(dtype);
			dispatch(dt, [&]<typename T>() { compressed::blosc2::ensure_mantissa_bits<T>(mantissa); return 0; });
			std::vector<device_view> views;
			if (py::isinstance<py::list>(channels) || py::isinstance<py::tuple>(channels))
				for (auto o : channels) views.push_back(view_of(py::reinterpret_borrow<py::object>(o), "DeviceImage"));
			else
			{
				device_view all = view_of(channels, "DeviceImage");
				if (all.shape.size() != 3) throw py::value_error("DeviceImage: a single array must have the shape (channels, height, width)");
				const size_t plane = static_cast<size_t>(all.shape[1] * all.shape[2]) * static_cast<size_t>(all.dt.itemsize());
				for (py::ssize_t k = 0; k < all.shape[0]; ++k)
				{
					device_view v = all;
					v.shape = { all.shape[1], all.shape[2] };
					v.ptr = static_cast<char*>(all.ptr) + static_cast<size_t>(k) * plane;
					views.push_back(v);
				}
			}
			return DeviceImage{ dispatch(dt, [&]<typename T>() -> any_dimage {
				std::vector<const T*> ptrs;
				for (const auto& v : views)
				{
					if (!v.dt.is(np_dtype<T>())) throw py::value_error("channel dtype does not match the image dtype");
					if (v.count() != width * height)
						throw py::value_error("Invalid channel data passed. Expected its size to match up to width * height (" + std::to_string(width * height) + "), got " + std::to_string(v.count()));
					ptrs.push_back(static_cast<const T*>(v.ptr));
				}
				wait_for(stream);
				return std::make_shared<compressed::device_image<T>>(ptrs, width, height, std::move(names), c, level, block, chunk, mantissa);
			}) };
		}
		static DeviceImage from_interleaved(const py::object& array, std::vector<std::string> names, codec c, size_t level, size_t block, size_t chunk,
			std::optional<uintptr_t> stream, std::optional<int> mantissa)
		{
			const device_view v = view_of(array, "from_interleaved");
			if (v.shape.size() != 3) throw py::value_error("from_interleaved: expected an array of the shape (height, width, channels)");
			return DeviceImage{ dispatch(v.dt, [&]<typename T>() -> any_dimage {
				compressed::blosc2::ensure_mantissa_bits<T>(mantissa);
				wait_for(stream);
				return std::make_shared<compressed::device_image<T>>(compressed::device_image<T>::from_interleaved(static_cast<const T*>(v.ptr),
					static_cast<size_t>(v.shape[1]), static_cast<size_t>(v.shape[0]), static_cast<size_t>(v.shape[2]), std::move(names), c, level, block, chunk, mantissa));
			}) };
		}
		static DeviceImage from_image(const Image& host)
		{
			return DeviceImage{ host.visit([]<typename T>(const img_ptr<T>& img) -> any_dimage {
				return std::make_shared<compressed::device_image<T>>(compressed::device_image<T>::from_image(*img)); }) };
		}
		Image to_image() const
		{
			return visit([]<typename T>(const dimg_ptr<T>& img) { return Image(any_image(std::make_shared<compressed::image<T>>(img->to_image()))); });
		}
		DeviceChannel channel(const std::variant<std::string, size_t>& key) const
		{
			return visit([&]<typename T>(const dimg_ptr<T>& img) {
				return DeviceChannel{ std::make_shared<compressed::device_channel<T>>(std::holds_alternative<size_t>(key) ? img->channel(std::get<size_t>(key))
					: img->channel(std::string_view(std::get<std::string>(key)))) };
			});
		}
		py::object get_decompressed(const py::object& out, std::optional<uintptr_t> stream) const
		{
			return visit([&]<typename T>(const dimg_ptr<T>& img) {
				auto [p, ret] = result_target<T>(out, { static_cast<py::ssize_t>(img->num_channels()), static_cast<py::ssize_t>(img->height()),
					static_cast<py::ssize_t>(img->width()) }, "get_decompressed");
				wait_for(stream);
				img->decompress_into(p);
				return ret;
			});
		}
		py::object get_region(py::ssize_t x, py::ssize_t y, py::ssize_t width, py::ssize_t height, const py::object& out, bool interleaved,
			std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y, const py::object& dtype, const py::object& scale,
			const py::object& offset) const
		{
			check_region_args(x, y, width, height);
			check_steps(step_x, step_y);
			return visit([&]<typename T>(const dimg_ptr<T>& img) -> py::object {
				const std::vector<float> sc = float_list(scale, img->num_channels(), "scale"), of = float_list(offset, img->num_channels(), "offset");
				if (dtype.is_none()) require_plain(sc, of, "get_region");
				if (img->num_channels()) img->channel(0).check_region(static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height));
				const py::ssize_t C = static_cast<py::ssize_t>(img->num_channels()), oh = ceil_div(height, step_y), ow = ceil_div(width, step_x);
				if (!dtype.is_none())
					return typed_dispatch<T>(dtype, [&]<typename U>() -> py::object {
						auto [p, ret] = result_target<U>(out, interleaved ? std::vector<py::ssize_t>{ oh, ow, C } : std::vector<py::ssize_t>{ C, oh, ow }, "get_region");
						wait_for(stream);
						img->get_region(p, static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height),
							static_cast<size_t>(step_x), static_cast<size_t>(step_y), std::span<const float>(sc), std::span<const float>(of), interleaved);
						return ret;
					}, "get_region");
				auto [p, ret] = result_target<T>(out, interleaved ? std::vector<py::ssize_t>{ oh, ow, C } : std::vector<py::ssize_t>{ C, oh, ow }, "get_region");
				wait_for(stream);
				if (step_x == 1 && step_y == 1)
					img->get_region(p, static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height), interleaved);
				else
					img->get_region(p, static_cast<size_t>(x), static_cast<size_t>(y), static_cast<size_t>(width), static_cast<size_t>(height),
						static_cast<size_t>(step_x), static_cast<size_t>(step_y), interleaved);
				return ret;
			});
		}
		// Image.get_regions / get_pixels into device memory: `out` or a new DeviceArray
		// (interleaved: (N, oh, ow, C) -- with or without dtype= a typed call, which places each channel's elements in its slots)
		py::object get_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, const py::object& out,
			std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y, bool pixels, const py::object& dtype = py::none(),
			const py::object& scale = py::float_(1.0), const py::object& offset = py::float_(0.0), bool interleaved = false) const
		{
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			const char* what = pixels ? "get_pixels" : "get_regions";
			return visit([&]<typename T>(const dimg_ptr<T>& img) -> py::object {
				const std::vector<float> sc = float_list(scale, img->num_channels(), "scale"), of = float_list(offset, img->num_channels(), "offset");
				if (dtype.is_none()) require_plain(sc, of, what);
				if (img->num_channels()) img->channel(0).check_regions(regions);
				if (!dtype.is_none() || interleaved)
				{
					const py::object want = dtype.is_none() ? py::object(np_dtype<T>()) : dtype;
					return typed_dispatch<T>(want, [&]<typename U>() -> py::object {
						std::vector<py::ssize_t> shape = regions_shape(regions.size(), img->num_channels(), width, height, step_x, step_y, pixels);
						if (interleaved && !pixels) shape = { shape[0], shape[2], shape[3], shape[1] };
						auto [p, ret] = result_target<U>(out, shape, what);
						wait_for(stream);
						img->get_regions(p, std::span<const compressed::region>(regions), std::span<const float>(sc), std::span<const float>(of), interleaved);
						return ret;
					}, what);
				}
				auto [p, ret] = result_target<T>(out, regions_shape(regions.size(), img->num_channels(), width, height, step_x, step_y, pixels),
					pixels ? "get_pixels" : "get_regions");
				wait_for(stream);
				img->get_regions(p, regions);
				return ret;
			});
		}
		// one (C, h', w') device array over every step_y-th row and step_x-th element from (x, y) of every channel
		// (dtype=: the array holds float32, float16 or the stored type, converted in the patch launch with one scale / offset or one per
		// channel; interleaved: the array is pixel-major, (h', w', C))
		void set_region(py::ssize_t x, py::ssize_t y, const py::object& array, std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y,
			const py::object& dtype = py::none(), const py::object& scale = py::float_(1.0), const py::object& offset = py::float_(0.0),
			bool interleaved = false)
		{
			if (x < 0 || y < 0) throw py::value_error("region coordinates must be >= 0");
			check_steps(step_x, step_y);
			if (dtype.is_none() && interleaved) throw py::value_error("set_region: interleaved needs dtype= (float32, float16 or the stored dtype)");
			const device_view v = view_of(array, "set_region");
			visit([&]<typename T>(const dimg_ptr<T>& img) {
				const std::vector<float> sc = float_list(scale, img->num_channels(), "scale"), of = float_list(offset, img->num_channels(), "offset");
				if (dtype.is_none()) require_plain(sc, of, "set_region");
				else
				{
					typed_source_dispatch<T>(dtype, v.dt, [&]<typename U>() {
						const size_t ci = interleaved ? 2 : 0, hi = interleaved ? 0 : 1, wi = interleaved ? 1 : 2;
						if (v.shape.size() != 3 || static_cast<size_t>(v.shape[ci]) != img->num_channels())
							throw py::value_error(interleaved ? "region arrays must have the shape (height, width, channels)" : "region arrays must have the shape (channels, height, width)");
						const size_t w = covered(v.shape[wi], step_x), h = covered(v.shape[hi], step_y);
						if (img->num_channels()) img->channel(0).check_region(static_cast<size_t>(x), static_cast<size_t>(y), w, h);
						wait_for(stream);
						img->set_region(static_cast<const U*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h, static_cast<size_t>(step_x),
							static_cast<size_t>(step_y), std::span<const float>(sc), std::span<const float>(of), interleaved);
					}, "set_region");
					return 0;
				}
				if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the image dtype");
				if (v.shape.size() != 3 || static_cast<size_t>(v.shape[0]) != img->num_channels())
					throw py::value_error("region arrays must have the shape (channels, height, width)");
				const size_t w = covered(v.shape[2], step_x), h = covered(v.shape[1], step_y);
				if (img->num_channels()) img->channel(0).check_region(static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				wait_for(stream);
				if (step_x == 1 && step_y == 1)
					img->set_region(static_cast<const T*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h);
				else
					img->set_region(static_cast<const T*>(v.ptr), static_cast<size_t>(x), static_cast<size_t>(y), w, h, static_cast<size_t>(step_x),
						static_cast<size_t>(step_y));
				return 0;
			});
		}
		// set_region / set_regions of every channel through ONE shared matte in device memory: array (C, h', w') / (N, C, h', w'),
		// mask (h', w') / (N, h', w'), bool or uint8
		void set_regions_masked(const py::object& xs, const py::object& ys, const py::object& arrays, std::optional<uintptr_t> stream, py::ssize_t step_x,
			py::ssize_t step_y, const py::object& masks, bool single)
		{
			const char* what = single ? "set_region" : "set_regions";
			check_steps(step_x, step_y);
			const device_view v = view_of(arrays, what);
			const size_t nd = single ? 3 : 4;
			if (v.shape.size() != nd) throw py::value_error(std::string(what) + (single ? ": region arrays must have the shape (channels, height, width)" : ": arrays must have the shape (N, channels, height, width)"));
			const auto regions = region_list(xs, ys, static_cast<py::ssize_t>(covered(v.shape[nd - 1], step_x)), static_cast<py::ssize_t>(covered(v.shape[nd - 2], step_y)),
				step_x, step_y);
			if (!single && regions.size() != static_cast<size_t>(v.shape[0]))
				throw py::value_error(std::string(what) + ": got " + std::to_string(v.shape[0]) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(const dimg_ptr<T>& img) {
				if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the image dtype");
				if (static_cast<size_t>(v.shape[nd - 3]) != img->num_channels()) throw py::value_error(std::string(what) + ": the arrays' channel count does not match the image");
				std::vector<py::ssize_t> mshape{ v.shape[nd - 2], v.shape[nd - 1] };
				if (!single) mshape.insert(mshape.begin(), v.shape[0]);
				const uint8_t* m = device_mask(masks, mshape, what);
				if (img->num_channels()) img->channel(0).check_regions(regions);
				if (regions.empty() || v.count() == 0) return 0;
				wait_for(stream);
				img->set_regions(std::span<const compressed::region>(regions), static_cast<const T*>(v.ptr), m);
				return 0;
			});
		}
		// fill_region / fill_regions of every channel: value a number or C numbers; masks (h', w') / (N, h', w') in device memory, shared
		void fill_regions(const py::object& xs, const py::object& ys, py::ssize_t width, py::ssize_t height, const py::object& value,
			std::optional<uintptr_t> stream, py::ssize_t step_x, py::ssize_t step_y, const py::object& masks, bool single)
		{
			const char* what = single ? "fill_region" : "fill_regions";
			const auto regions = region_list(xs, ys, width, height, step_x, step_y);
			visit([&]<typename T>(const dimg_ptr<T>& img) {
				const std::vector<T> values = fill_values<T>(value, img->num_channels(), what);
				std::vector<py::ssize_t> shape{ ceil_div(height, step_y), ceil_div(width, step_x) };
				if (!single) shape.insert(shape.begin(), static_cast<py::ssize_t>(regions.size()));
				const uint8_t* m = masks.is_none() ? nullptr : device_mask(masks, shape, what);
				if (img->num_channels()) img->channel(0).check_regions(regions);
				if (regions.empty() || width == 0 || height == 0) return 0;
				wait_for(stream);
				if (m) img->fill_regions(std::span<const compressed::region>(regions), std::span<const T>(values), m);
				else img->fill_regions(std::span<const compressed::region>(regions), std::span<const T>(values));
				return 0;
			});
		}
		// arrays: (N, C, h', w') in device memory (pixels: (N, C)), region k from (xs[k], ys[k]) of every channel; later regions win
		// (dtype=: converted in the patch launch; interleaved: (N, h', w', C) -- pixels are (N, C) either way)
		void set_regions(const py::object& xs, const py::object& ys, const py::object& arrays, std::optional<uintptr_t> stream, py::ssize_t step_x,
			py::ssize_t step_y, bool pixels, const py::object& dtype = py::none(), const py::object& scale = py::float_(1.0),
			const py::object& offset = py::float_(0.0), bool interleaved = false)
		{
			const char* what = pixels ? "set_pixels" : "set_regions";
			check_steps(step_x, step_y);
			if (dtype.is_none() && interleaved) throw py::value_error(std::string(what) + ": interleaved needs dtype= (float32, float16 or the stored dtype)");
			const device_view v = view_of(arrays, what);
			const bool pm = interleaved && !pixels;                       // (N, h', w', C)
			if (v.shape.size() != (pixels ? 2u : 4u))
				throw py::value_error(std::string(what) + (pixels ? ": values must have the shape (N, channels)" : pm ? ": arrays must have the shape (N, height, width, channels)" : ": arrays must have the shape (N, channels, height, width)"));
			const size_t ci = pm ? 3 : 1;
			const auto regions = region_list(xs, ys, pixels ? 1 : static_cast<py::ssize_t>(covered(v.shape[pm ? 2 : 3], step_x)),
				pixels ? 1 : static_cast<py::ssize_t>(covered(v.shape[pm ? 1 : 2], step_y)), step_x, step_y);
			if (regions.size() != static_cast<size_t>(v.shape[0]))
				throw py::value_error(std::string(what) + ": got " + std::to_string(v.shape[0]) + " arrays for " + std::to_string(regions.size()) + " coordinates");
			visit([&]<typename T>(const dimg_ptr<T>& img) {
				const std::vector<float> sc = float_list(scale, img->num_channels(), "scale"), of = float_list(offset, img->num_channels(), "offset");
				if (dtype.is_none()) require_plain(sc, of, what);
				else
				{
					typed_source_dispatch<T>(dtype, v.dt, [&]<typename U>() {
						if (static_cast<size_t>(v.shape[ci]) != img->num_channels()) throw py::value_error(std::string(what) + ": the arrays' channel count does not match the image");
						if (img->num_channels()) img->channel(0).check_regions(regions);
						wait_for(stream);
						img->set_regions(std::span<const compressed::region>(regions), static_cast<const U*>(v.ptr), std::span<const float>(sc),
							std::span<const float>(of), interleaved);
					}, what);
					return 0;
				}
				if (!v.dt.is(np_dtype<T>())) throw py::value_error("array dtype does not match the image dtype");
				if (static_cast<size_t>(v.shape[1]) != img->num_channels()) throw py::value_error(std::string(what) + ": the arrays' channel count does not match the image");
				if (img->num_channels()) img->channel(0).check_regions(regions);
				if (regions.empty() || v.count() == 0) return 0;
				wait_for(stream);
				img->set_regions(regions, static_cast<const T*>(v.ptr));
				return 0;
			});
		}
	};
}

PYBIND11_MODULE(compressed_image, m)
{
	m.doc() = "MI355X-native chunked image compression (drop-in for EmilDohne/compressed-image's Python module)";

	py::enum_<codec>(m, "Codec", py::module_local())
		.value("blosclz", codec::blosclz)
		.value("lz4", codec::lz4)
		.value("lz4hc", codec::lz4hc)
		.value("zstd", codec::zstd)
		.export_values();

	const auto d_block = compressed::s_default_blocksize, d_chunk = compressed::s_default_chunksize;

	py::class_<Channel>(m, "Channel", py::module_local())
		.def(py::init(&Channel::from_array), py::arg("data"), py::arg("width"), py::arg("height"), py::arg("compression_codec") = codec::lz4,
			py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk, py::arg("mantissa_bits") = std::nullopt)
		.def("mantissa_bits", &Channel::mantissa_bits)
		.def_static("full", &Channel::full, py::arg("dtype"), py::arg("fill_value"), py::arg("width"), py::arg("height"),
			py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk)
		.def_static("zeros", [](const py::object& dtype, size_t w, size_t h, codec c, size_t level, size_t block, size_t chunk) {
				return Channel::full(dtype, py::int_(0), w, h, c, level, block, chunk); },
			py::arg("dtype"), py::arg("width"), py::arg("height"), py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9,
			py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk)
		.def_static("full_like", &Channel::full_like, py::arg("other"), py::arg("fill_value"))
		.def_static("zeros_like", [](const Channel& other) { return Channel::full_like(other, py::int_(0)); }, py::arg("other"))
		.def_property_readonly("dtype", &Channel::dtype)
		.def_property_readonly("shape", [](const Channel& c) { return py::make_tuple(c.height(), c.width()); })
		.def_property_readonly("width", &Channel::width)
		.def_property_readonly("height", &Channel::height)
		.def("block_size", [](const Channel& c) { return c.visit([](auto& ch) { return ch.block_size(); }); })
		.def("chunk_size", [](const Channel& c) { return c.visit([](auto& ch) { return ch.chunk_size(); }); })
		.def("chunk_size", [](const Channel& c, size_t i) { return c.visit([&](auto& ch) { return ch.chunk_size(i); }); }, py::arg("chunk_index"))
		.def("chunk_elems", [](const Channel& c) { return c.visit([](auto& ch) { return ch.chunk_elems(); }); })
		.def("chunk_elems", [](const Channel& c, size_t i) { return c.visit([&](auto& ch) { return ch.chunk_elems(i); }); }, py::arg("chunk_index"))
		.def("compressed_bytes", [](const Channel& c) { return c.visit([](auto& ch) { return ch.compressed_bytes(); }); })
		.def("uncompressed_size", [](const Channel& c) { return c.visit([](auto& ch) { return ch.uncompressed_size(); }); })
		.def("num_chunks", [](const Channel& c) { return c.visit([](auto& ch) { return ch.num_chunks(); }); })
		.def("compression", [](const Channel& c) { return c.visit([](auto& ch) { return ch.compression(); }); })
		.def("compression_level", [](const Channel& c) { return c.visit([](auto& ch) { return static_cast<size_t>(ch.compression_level()); }); })
		.def("update_nthreads", [](Channel& c, size_t n, size_t block) { c.visit([&](auto& ch) { ch.update_nthreads(n, block); return 0; }); },
			py::arg("nthreads"), py::arg("block_size") = d_block)
		.def("get_chunk", &Channel::get_chunk, py::arg("chunk_index"))
		.def("get_chunk", &Channel::get_chunk_into, py::arg("chunk_index"), py::arg("array"))
		.def("set_chunk", &Channel::set_chunk, py::arg("chunk_index"), py::arg("array"))
		.def("get_decompressed", &Channel::get_decompressed)
		.def("get_region", &Channel::get_region, py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("step_x") = 1,
			py::arg("step_y") = 1)
		.def("get_regions", [](const Channel& c, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, py::ssize_t sx, py::ssize_t sy) {
				return c.get_regions(xs, ys, w, h, sx, sy, false); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("step_x") = 1, py::arg("step_y") = 1)
		.def("get_pixels", [](const Channel& c, const py::object& xs, const py::object& ys) { return c.get_regions(xs, ys, 1, 1, 1, 1, true); },
			py::arg("xs"), py::arg("ys"))
		.def("__getitem__", &Channel::getitem, py::arg("key"))
		.def("set_region", [](Channel& c, py::ssize_t x, py::ssize_t y, const py::array& array, py::ssize_t sx, py::ssize_t sy, const py::object& mask) {
				if (mask.is_none()) c.set_region(x, y, array, sx, sy);
				else c.set_regions_masked(py::make_tuple(x), py::make_tuple(y), array, sx, sy, mask, true); },
			py::arg("x"), py::arg("y"), py::arg("array"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("mask") = py::none())
		.def("set_regions", [](Channel& c, const py::object& xs, const py::object& ys, const py::array& arrays, py::ssize_t sx, py::ssize_t sy, const py::object& masks) {
				if (masks.is_none()) c.set_regions(xs, ys, arrays, sx, sy, false);
				else c.set_regions_masked(xs, ys, arrays, sx, sy, masks, false); },
			py::arg("xs"), py::arg("ys"), py::arg("arrays"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("masks") = py::none())
		.def("fill_region", [](Channel& c, py::ssize_t x, py::ssize_t y, py::ssize_t w, py::ssize_t h, const py::object& value, py::ssize_t sx, py::ssize_t sy,
				const py::object& mask) { check_region_args(x, y, w, h); c.fill_regions(py::make_tuple(x), py::make_tuple(y), w, h, value, sx, sy, mask, true); },
			py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("mask") = py::none())
		.def("fill_regions", [](Channel& c, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, const py::object& value, py::ssize_t sx,
				py::ssize_t sy, const py::object& masks) { c.fill_regions(xs, ys, w, h, value, sx, sy, masks, false); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("masks") = py::none())
		.def("set_pixels", [](Channel& c, const py::object& xs, const py::object& ys, const py::array& values) { c.set_regions(xs, ys, values, 1, 1, true); },
			py::arg("xs"), py::arg("ys"), py::arg("values"))
		.def("__setitem__", &Channel::setitem, py::arg("key"), py::arg("value"));

	py::class_<Image>(m, "Image", py::module_local())
		.def(py::init<const py::object&, const std::vector<py::array>&, size_t, size_t, std::vector<std::string>, codec, size_t, size_t, size_t, std::optional<int>>(),
			py::arg("dtype"), py::arg("channels"), py::arg("width"), py::arg("height"), py::arg("channel_names") = std::vector<std::string>{},
			py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk,
			py::arg("mantissa_bits") = std::nullopt)
		.def("mantissa_bits", [](const Image& i) { return i.visit([](auto& img) { return img->mantissa_bits(); }); })
		.def("add_channel", &Image::add_channel, py::arg("data"), py::arg("width"), py::arg("height"), py::arg("name") = std::nullopt,
			py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk,
			py::arg("mantissa_bits") = std::nullopt)
		.def("remove_channel", &Image::remove_channel, py::arg("name_or_index"))
		.def("__getitem__", &Image::channel, py::arg("key"))
		.def("__len__", [](const Image& i) { return i.visit([](auto& img) { return img->num_channels(); }); })
		.def("channel", &Image::channel, py::arg("key"))
		.def("channels", &Image::channels)
		.def("get_decompressed", &Image::get_decompressed)
		.def("get_region", &Image::get_region, py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("step_x") = 1,
			py::arg("step_y") = 1)
		.def("get_regions", [](const Image& i, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, py::ssize_t sx, py::ssize_t sy) {
				return i.get_regions(xs, ys, w, h, sx, sy, false); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("step_x") = 1, py::arg("step_y") = 1)
		.def("get_pixels", [](const Image& i, const py::object& xs, const py::object& ys) { return i.get_regions(xs, ys, 1, 1, 1, 1, true); },
			py::arg("xs"), py::arg("ys"))
		.def("set_region", [](Image& i, py::ssize_t x, py::ssize_t y, const std::vector<py::array>& arrays, py::ssize_t sx, py::ssize_t sy, const py::object& mask) {
				if (mask.is_none()) { i.set_region(x, y, arrays, sx, sy); return; }
				if (x < 0 || y < 0) throw py::value_error("region coordinates must be >= 0");
				i.set_regions_masked(py::make_tuple(x), py::make_tuple(y), py::cast(arrays), sx, sy, mask, true); },
			py::arg("x"), py::arg("y"), py::arg("arrays"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("mask") = py::none())
		.def("set_regions", [](Image& i, const py::object& xs, const py::object& ys, const py::array& arrays, py::ssize_t sx, py::ssize_t sy, const py::object& masks) {
				if (masks.is_none()) i.set_regions(xs, ys, arrays, sx, sy, false);
				else i.set_regions_masked(xs, ys, arrays, sx, sy, masks, false); },
			py::arg("xs"), py::arg("ys"), py::arg("arrays"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("masks") = py::none())
		.def("fill_region", [](Image& i, py::ssize_t x, py::ssize_t y, py::ssize_t w, py::ssize_t h, const py::object& value, py::ssize_t sx, py::ssize_t sy,
				const py::object& mask) { check_region_args(x, y, w, h); i.fill_regions(py::make_tuple(x), py::make_tuple(y), w, h, value, sx, sy, mask, true); },
			py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("mask") = py::none())
		.def("fill_regions", [](Image& i, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, const py::object& value, py::ssize_t sx,
				py::ssize_t sy, const py::object& masks) { i.fill_regions(xs, ys, w, h, value, sx, sy, masks, false); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("masks") = py::none())
		.def("set_pixels", [](Image& i, const py::object& xs, const py::object& ys, const py::array& values) { i.set_regions(xs, ys, values, 1, 1, true); },
			py::arg("xs"), py::arg("ys"), py::arg("values"))
		.def("get_channel_index", [](const Image& i, const std::string& name) { return i.visit([&](auto& img) { return img->get_channel_offset(name); }); }, py::arg("channelname"))
		.def("print_statistics", [](const Image& i) { i.visit([](auto& img) { img->print_statistics(); return 0; }); })
		.def("compression_ratio", [](const Image& i) { return i.visit([](auto& img) { return img->compression_ratio(); }); })
		.def_property_readonly("dtype", [](const Image& i) { return i.visit([]<typename T>(const img_ptr<T>&) { return np_dtype<T>(); }); })
		.def_property_readonly("shape", [](const Image& i) { return i.visit([](auto& img) { return py::make_tuple(img->num_channels(), img->height(), img->width()); }); })
		.def_property_readonly("width", [](const Image& i) { return i.visit([](auto& img) { return img->width(); }); })
		.def_property_readonly("height", [](const Image& i) { return i.visit([](auto& img) { return img->height(); }); })
		.def_property_readonly("num_channels", [](const Image& i) { return i.visit([](auto& img) { return img->num_channels(); }); })
		.def("get_channel_names", [](const Image& i) { return i.visit([](auto& img) { return img->channelnames(); }); })
		.def("set_channel_names", [](Image& i, std::vector<std::string> names) { i.visit([&](auto& img) { img->channelnames(std::move(names)); return 0; }); }, py::arg("channel_names"))
		.def("update_nthreads", [](Image& i, size_t n) { i.visit([&](auto& img) { img->update_nthreads(n); return 0; }); }, py::arg("nthreads"))
		.def("block_size", [](const Image& i) { return i.visit([](auto& img) { return img->block_size(); }); })
		.def("chunk_size", [](const Image& i) { return i.visit([](auto& img) { return img->chunk_size(); }); })
		.def("set_metadata", [](Image& i, py::dict md) { i.metadata = std::move(md); }, py::arg("metadata"))
		.def("get_metadata", [](const Image& i) { return i.metadata; });

	py::class_<DeviceArray>(m, "DeviceArray", py::module_local())
		.def_property_readonly("__cuda_array_interface__", &DeviceArray::interface)
		.def_property_readonly("shape", [](const DeviceArray& a) { return py::tuple(py::cast(a.shape)); })
		.def_property_readonly("dtype", [](const DeviceArray& a) { return a.dt; })
		.def_property_readonly("nbytes", [](const DeviceArray& a) { return a.nbytes; })
		.def("copy_to_host", &DeviceArray::copy_to_host);

	py::class_<DeviceChannel>(m, "DeviceChannel", py::module_local())
		.def(py::init(&DeviceChannel::from_array), py::arg("data"), py::arg("width"), py::arg("height"), py::arg("compression_codec") = codec::lz4,
			py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk, py::arg("stream") = std::nullopt,
			py::arg("mantissa_bits") = std::nullopt)
		.def("mantissa_bits", &DeviceChannel::mantissa_bits)
		.def_static("from_channel", &DeviceChannel::from_channel, py::arg("channel"))
		.def_static("full", &DeviceChannel::full, py::arg("dtype"), py::arg("fill_value"), py::arg("width"), py::arg("height"),
			py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk,
			py::arg("mantissa_bits") = std::nullopt)
		.def_static("zeros", [](const py::object& dtype, size_t w, size_t h, codec c, size_t level, size_t block, size_t chunk, std::optional<int> mantissa) {
				return DeviceChannel::full(dtype, py::int_(0), w, h, c, level, block, chunk, mantissa); },
			py::arg("dtype"), py::arg("width"), py::arg("height"), py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9,
			py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk, py::arg("mantissa_bits") = std::nullopt)
		.def_static("full_like", &DeviceChannel::full_like, py::arg("other"), py::arg("fill_value"))
		.def_static("zeros_like", [](const DeviceChannel& other) { return DeviceChannel::full_like(other, py::int_(0)); }, py::arg("other"))
		.def("to_channel", &DeviceChannel::to_channel)
		.def_property_readonly("dtype", [](const DeviceChannel& c) { return c.visit([]<typename T>(compressed::device_channel<T>&) { return np_dtype<T>(); }); })
		.def_property_readonly("shape", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return py::make_tuple(ch.height(), ch.width()); }); })
		.def_property_readonly("width", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.width(); }); })
		.def_property_readonly("height", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.height(); }); })
		.def("block_size", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.block_size(); }); })
		.def("chunk_size", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.chunk_size(); }); })
		.def("chunk_size", [](const DeviceChannel& c, size_t i) { return c.visit([&](auto& ch) { return ch.chunk_size(i); }); }, py::arg("chunk_index"))
		.def("chunk_elems", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.chunk_elems(); }); })
		.def("chunk_elems", [](const DeviceChannel& c, size_t i) { return c.visit([&](auto& ch) { return ch.chunk_elems(i); }); }, py::arg("chunk_index"))
		.def("compressed_bytes", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.compressed_bytes(); }); })
		.def("compressed_bytes", [](const DeviceChannel& c, size_t i) { return c.visit([&](auto& ch) { return ch.compressed_bytes(i); }); }, py::arg("chunk_index"))
		.def("uncompressed_size", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.uncompressed_size(); }); })
		.def("num_chunks", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.num_chunks(); }); })
		.def("compression", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.compression(); }); })
		.def("compression_level", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return static_cast<size_t>(ch.compression_level()); }); })
		.def("device_bytes", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.device_bytes(); }); })
		.def("read_only", [](const DeviceChannel& c) { return c.visit([](auto& ch) { return ch.read_only(); }); })
		.def("get_decompressed", &DeviceChannel::get_decompressed, py::arg("out") = py::none(), py::arg("stream") = std::nullopt)
		.def("get_region", &DeviceChannel::get_region, py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("out") = py::none(),
			py::arg("stream") = std::nullopt, py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("dtype") = py::none(), py::arg("scale") = 1.0,
			py::arg("offset") = 0.0)
		.def("get_regions", [](const DeviceChannel& c, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, const py::object& out,
				std::optional<uintptr_t> stream, py::ssize_t sx, py::ssize_t sy, const py::object& dtype, const py::object& scale, const py::object& offset) {
				return c.get_regions(xs, ys, w, h, out, stream, sx, sy, false, dtype, scale, offset); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("out") = py::none(), py::arg("stream") = std::nullopt,
			py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("dtype") = py::none(), py::arg("scale") = 1.0, py::arg("offset") = 0.0)
		.def("get_pixels", [](const DeviceChannel& c, const py::object& xs, const py::object& ys, const py::object& out, std::optional<uintptr_t> stream,
				const py::object& dtype, const py::object& scale, const py::object& offset) {
				return c.get_regions(xs, ys, 1, 1, out, stream, 1, 1, true, dtype, scale, offset); },
			py::arg("xs"), py::arg("ys"), py::arg("out") = py::none(), py::arg("stream") = std::nullopt, py::arg("dtype") = py::none(),
			py::arg("scale") = 1.0, py::arg("offset") = 0.0)
		.def("__getitem__", &DeviceChannel::getitem, py::arg("key"))
		.def("set_region", &DeviceChannel::set_region, py::arg("x"), py::arg("y"), py::arg("array"), py::arg("stream") = std::nullopt,
			py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("dtype") = py::none(), py::arg("scale") = 1.0, py::arg("offset") = 0.0,
			py::arg("mask") = py::none())
		.def("set_regions", [](DeviceChannel& c, const py::object& xs, const py::object& ys, const py::object& arrays, std::optional<uintptr_t> stream,
				py::ssize_t sx, py::ssize_t sy, const py::object& dtype, const py::object& scale, const py::object& offset, const py::object& masks) {
				c.set_regions(xs, ys, arrays, stream, sx, sy, false, dtype, scale, offset, masks); },
			py::arg("xs"), py::arg("ys"), py::arg("arrays"), py::arg("stream") = std::nullopt, py::arg("step_x") = 1, py::arg("step_y") = 1,
			py::arg("dtype") = py::none(), py::arg("scale") = 1.0, py::arg("offset") = 0.0, py::arg("masks") = py::none())
		.def("fill_region", &DeviceChannel::fill_region, py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("value"),
			py::arg("stream") = std::nullopt, py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("mask") = py::none())
		.def("fill_regions", [](DeviceChannel& c, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, const py::object& value,
				std::optional<uintptr_t> stream, py::ssize_t sx, py::ssize_t sy, const py::object& masks) {
				c.fill_regions(xs, ys, w, h, value, stream, sx, sy, masks); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("stream") = std::nullopt,
			py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("masks") = py::none())
		.def("set_pixels", [](DeviceChannel& c, const py::object& xs, const py::object& ys, const py::object& values, std::optional<uintptr_t> stream,
				const py::object& dtype, const py::object& scale, const py::object& offset) {
				c.set_regions(xs, ys, values, stream, 1, 1, true, dtype, scale, offset); },
			py::arg("xs"), py::arg("ys"), py::arg("values"), py::arg("stream") = std::nullopt, py::arg("dtype") = py::none(), py::arg("scale") = 1.0,
			py::arg("offset") = 0.0)
		.def("__setitem__", &DeviceChannel::setitem, py::arg("key"), py::arg("value"));

	py::class_<DeviceImage>(m, "DeviceImage", py::module_local())
		.def(py::init(&DeviceImage::from_arrays), py::arg("dtype"), py::arg("channels"), py::arg("width"), py::arg("height"),
			py::arg("channel_names") = std::vector<std::string>{}, py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9,
			py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk, py::arg("stream") = std::nullopt, py::arg("mantissa_bits") = std::nullopt)
		.def("mantissa_bits", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->mantissa_bits(); }); })
		.def_static("from_interleaved", &DeviceImage::from_interleaved, py::arg("array"), py::arg("channel_names") = std::vector<std::string>{},
			py::arg("compression_codec") = codec::lz4, py::arg("compression_level") = 9, py::arg("block_size") = d_block, py::arg("chunk_size") = d_chunk,
			py::arg("stream") = std::nullopt, py::arg("mantissa_bits") = std::nullopt)
		.def_static("from_image", &DeviceImage::from_image, py::arg("image"))
		.def("to_image", &DeviceImage::to_image)
		.def("__getitem__", &DeviceImage::channel, py::arg("key"))
		.def("__len__", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->num_channels(); }); })
		.def("channel", &DeviceImage::channel, py::arg("key"))
		.def("get_decompressed", &DeviceImage::get_decompressed, py::arg("out") = py::none(), py::arg("stream") = std::nullopt)
		.def("get_region", &DeviceImage::get_region, py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("out") = py::none(),
			py::arg("interleaved") = false, py::arg("stream") = std::nullopt, py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("dtype") = py::none(),
			py::arg("scale") = 1.0, py::arg("offset") = 0.0)
		.def("get_regions", [](const DeviceImage& i, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, const py::object& out,
				std::optional<uintptr_t> stream, py::ssize_t sx, py::ssize_t sy, const py::object& dtype, const py::object& scale, const py::object& offset,
				bool interleaved) { return i.get_regions(xs, ys, w, h, out, stream, sx, sy, false, dtype, scale, offset, interleaved); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("out") = py::none(), py::arg("stream") = std::nullopt,
			py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("dtype") = py::none(), py::arg("scale") = 1.0, py::arg("offset") = 0.0,
			py::arg("interleaved") = false)
		.def("get_pixels", [](const DeviceImage& i, const py::object& xs, const py::object& ys, const py::object& out, std::optional<uintptr_t> stream,
				const py::object& dtype, const py::object& scale, const py::object& offset) {
				return i.get_regions(xs, ys, 1, 1, out, stream, 1, 1, true, dtype, scale, offset); },
			py::arg("xs"), py::arg("ys"), py::arg("out") = py::none(), py::arg("stream") = std::nullopt, py::arg("dtype") = py::none(),
			py::arg("scale") = 1.0, py::arg("offset") = 0.0)
		.def("set_region", [](DeviceImage& i, py::ssize_t x, py::ssize_t y, const py::object& array, std::optional<uintptr_t> stream, py::ssize_t sx, py::ssize_t sy,
				const py::object& dtype, const py::object& scale, const py::object& offset, bool interleaved, const py::object& mask) {
				if (mask.is_none()) { i.set_region(x, y, array, stream, sx, sy, dtype, scale, offset, interleaved); return; }
				if (!dtype.is_none() || interleaved) throw py::value_error("set_region: mask= cannot be combined with dtype= or interleaved= (masked typed writes are not built)");
				if (x < 0 || y < 0) throw py::value_error("region coordinates must be >= 0");
				i.set_regions_masked(py::make_tuple(x), py::make_tuple(y), array, stream, sx, sy, mask, true); },
			py::arg("x"), py::arg("y"), py::arg("array"), py::arg("stream") = std::nullopt,
			py::arg("step_x") = 1, py::arg("step_y") = 1, py::arg("dtype") = py::none(), py::arg("scale") = 1.0, py::arg("offset") = 0.0,
			py::arg("interleaved") = false, py::arg("mask") = py::none())
		.def("set_regions", [](DeviceImage& i, const py::object& xs, const py::object& ys, const py::object& arrays, std::optional<uintptr_t> stream,
				py::ssize_t sx, py::ssize_t sy, const py::object& dtype, const py::object& scale, const py::object& offset, bool interleaved, const py::object& masks) {
				if (masks.is_none()) { i.set_regions(xs, ys, arrays, stream, sx, sy, false, dtype, scale, offset, interleaved); return; }
				if (!dtype.is_none() || interleaved) throw py::value_error("set_regions: masks= cannot be combined with dtype= or interleaved= (masked typed writes are not built)");
				i.set_regions_masked(xs, ys, arrays, stream, sx, sy, masks, false); },
			py::arg("xs"), py::arg("ys"), py::arg("arrays"), py::arg("stream") = std::nullopt, py::arg("step_x") = 1, py::arg("step_y") = 1,
			py::arg("dtype") = py::none(), py::arg("scale") = 1.0, py::arg("offset") = 0.0, py::arg("interleaved") = false, py::arg("masks") = py::none())
		.def("fill_region", [](DeviceImage& i, py::ssize_t x, py::ssize_t y, py::ssize_t w, py::ssize_t h, const py::object& value, std::optional<uintptr_t> stream,
				py::ssize_t sx, py::ssize_t sy, const py::object& mask) {
				check_region_args(x, y, w, h); i.fill_regions(py::make_tuple(x), py::make_tuple(y), w, h, value, stream, sx, sy, mask, true); },
			py::arg("x"), py::arg("y"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("stream") = std::nullopt, py::arg("step_x") = 1,
			py::arg("step_y") = 1, py::arg("mask") = py::none())
		.def("fill_regions", [](DeviceImage& i, const py::object& xs, const py::object& ys, py::ssize_t w, py::ssize_t h, const py::object& value,
				std::optional<uintptr_t> stream, py::ssize_t sx, py::ssize_t sy, const py::object& masks) { i.fill_regions(xs, ys, w, h, value, stream, sx, sy, masks, false); },
			py::arg("xs"), py::arg("ys"), py::arg("width"), py::arg("height"), py::arg("value"), py::arg("stream") = std::nullopt, py::arg("step_x") = 1,
			py::arg("step_y") = 1, py::arg("masks") = py::none())
		.def("set_pixels", [](DeviceImage& i, const py::object& xs, const py::object& ys, const py::object& values, std::optional<uintptr_t> stream,
				const py::object& dtype, const py::object& scale, const py::object& offset, bool interleaved) {
				i.set_regions(xs, ys, values, stream, 1, 1, true, dtype, scale, offset, interleaved); },
			py::arg("xs"), py::arg("ys"), py::arg("values"), py::arg("stream") = std::nullopt, py::arg("dtype") = py::none(), py::arg("scale") = 1.0,
			py::arg("offset") = 0.0, py::arg("interleaved") = false)
		.def("get_channel_index", [](const DeviceImage& i, const std::string& name) { return i.visit([&](auto& img) { return img->get_channel_offset(name); }); }, py::arg("channelname"))
		.def("get_channel_names", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->channelnames(); }); })
		.def("set_channel_names", [](DeviceImage& i, std::vector<std::string> names) { i.visit([&](auto& img) { img->channelnames(std::move(names)); return 0; }); }, py::arg("channel_names"))
		.def("compression_ratio", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->compression_ratio(); }); })
		.def_property_readonly("dtype", [](const DeviceImage& i) { return i.visit([]<typename T>(const dimg_ptr<T>&) { return np_dtype<T>(); }); })
		.def_property_readonly("shape", [](const DeviceImage& i) { return i.visit([](auto& img) { return py::make_tuple(img->num_channels(), img->height(), img->width()); }); })
		.def_property_readonly("width", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->width(); }); })
		.def_property_readonly("height", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->height(); }); })
		.def_property_readonly("num_channels", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->num_channels(); }); })
		.def("block_size", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->block_size(); }); })
		.def("chunk_size", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->chunk_size(); }); })
		.def("compressed_bytes", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->compressed_bytes(); }); })
		.def("uncompressed_size", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->uncompressed_size(); }); })
		.def("num_chunks", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->num_chunks(); }); })
		.def("device_bytes", [](const DeviceImage& i) { return i.visit([](auto& img) { return img->device_bytes(); }); });
}
