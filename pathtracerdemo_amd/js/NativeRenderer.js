'use strict';
/**
 * NativeRenderer -- the drop-in for the reference's Renderer_TEST
 * (apps/frontend/src/graphics-core/Renderer_TEST.ts) over the ptx_node N-API addon.
 *
 * Same surface: constructor, async Initialize(world), Update(), Render(), GetCamera(),
 * ResetFrameCount(); WebGPUEngine's loop (GC/service/WebGPUEngine.ts:199-200) calls
 * Update() then Render() per tick exactly as before, and nothing else.  Like Renderer_TEST.Render
 * (Renderer_TEST.ts:233-258, which ends by drawing into the canvas it was constructed with),
 * Render() paints the canvas it was given: when the canvas offers getContext('2d'), the reference's
 * render pass (the fullscreen quad + FragmentShader.wgsl's fixed 600 x 450 texel window, unorm8)
 * runs on the GPU behind the frame (ptx_present_async) and its bytes go to putImageData once they
 * have landed -- polled off the event loop, never waited for; while one present is in flight a
 * newer frame is presented after it, so the canvas always ends on the newest finished frame
 * (PresentedSerial: the Render() call it shows; PresentIdle(): a promise for "nothing in flight").
 * ReadImage / RenderAsync(out) give the accumulated RGBA f32 image; Present(canvasW, canvasH)
 * is the same render pass, blocking, into RGBA (putImageData) or BGRA (a bgra8unorm WebGPU
 * canvas) bytes.  presentImage does it on the host for a frame gathered from row bands
 * (renderBands).
 * Denoise(opts) enqueues ptx_denoise behind the frame last rendered; after
 * SetPresentSource('denoised') the canvas shows the denoised image: Render() then leaves the
 * painting to the Denoise() that follows it (call it after every Render(), before the next
 * Update()).  {frameColor: true} creates the handle with PTX_FLAG_FRAME_COLOR, which
 * Denoise({temporal: true}) needs.  The default source stays 'accum'.
 *
 * `world` is the reference's own World (./world.js: World.LoadFromScene over the Scene JSON,
 * meshes in ResourceManager.MeshPool), serialized here by SerializeWorldData exactly as
 * Renderer_TEST.CreateGPUResources does (Renderer_TEST.ts:445-460) -- or, equivalently, an
 * already serialized { scene, geometry, accel: Uint32Array, offsets: number[7],
 * instanceCount, lightCount } (scene_io.loadCompiledScene reads one from disk).
 * There is no CPU fallback: a missing addon or libptx.so throws at require time.
 */
const path = require('path');
const { Camera } = require('./Camera');
const { mat4 } = require('./wgpu_math');
const { SerializeWorldData } = require('./world');

const addon = require(path.join(__dirname, '..', 'ptx_node.node'));

const PIPELINE = { restir: 0, mcpt: 1, reuse: 2, gi: 3 };
const PASS = { GBUFFER: 0, INIT: 1, FINAL: 2, MCPT: 3, TRACE: 4, WAVE_TRACE: 5, WAVE_LOGIC: 6, FRAME: 7,
  TEMPORAL: 8, SPATIAL: 9, PASS_GROUP: 10 };
const BUF = { GBUFFER: 0, RESERVOIR: 1, ACCUM: 2, COUNTERS: 3, RESERVOIR_HIST: 4, DIRECT: 5, DENOISED: 6, FRAME_COLOR: 7,
  DENOISE_HISTORY: 8, UPSAMPLE_HISTORY: 9 };
const FLAGS = { COUNT_WORK: 1, SIMPLE_KERNELS: 2, TIME_LAUNCHES: 16, FRAME_COLOR: 512 };
const UNIFORM_WORDS = 33;

/** The 33-word uniform block of Renderer_TEST.Update (Renderer_TEST.ts:165-206). */
function buildUniform(width, height, camera, frameCount, world) {
  const data = new ArrayBuffer(4 * UNIFORM_WORDS);
  const f32 = new Float32Array(data);
  const u32 = new Uint32Array(data);
  const loc = camera.GetLocation();
  const vpInv = mat4.invert(camera.GetViewProjectionMatrix());
  u32[0] = width;
  u32[1] = height;
  u32[2] = 10; // Max Bounce (unused by the kernels)
  u32[3] = 1;  // SPP
  for (let i = 0; i < 16; i++) f32[4 + i] = vpInv[i];
  f32[20] = loc[0];
  f32[21] = loc[1];
  f32[22] = loc[2];
  u32[23] = frameCount;
  for (let i = 0; i < 7; i++) u32[24 + i] = world.offsets[i];
  u32[31] = world.instanceCount;
  u32[32] = world.lightCount;
  return u32;
}

function isCanvas(x) {
  return !!x && typeof x === 'object' && typeof x.width === 'number' && typeof x.height === 'number';
}

// the next turn of the event loop (Node: setImmediate; a browser: a zero timeout)
const soon = typeof setImmediate === 'function' ? setImmediate : (fn) => setTimeout(fn, 0);

class NativeRenderer {
  /**
   * Three call forms:
   *   new NativeRenderer(adapter, device, canvas, [options])  -- Renderer_TEST's own
   *     (Renderer_TEST.ts:83-88, WebGPUEngine.ts:83); adapter / device are not used;
   *   new NativeRenderer(canvas, [options]);
   *   new NativeRenderer(width, height, [options]).
   * `canvas` is anything with numeric width / height (an HTMLCanvasElement, an OffscreenCanvas,
   * a plain object): like Renderer_TEST, Initialize() reads its size each time it is called, so
   * WebGPUEngine.resize (set canvas.width / height, then Initialize(world), WebGPUEngine.ts:132-142)
   * recreates the handle at the new size.
   * @param {object} [options] {pipeline: 'restir'|'mcpt'|'reuse'|'gi', device, rowBegin, rowEnd, flags,
   *   reuseRadius, reuseNeighbors, temporalCap, frameColor}
   */
  constructor(a, b, c, d) {
    let options;
    if (typeof a === 'number') {
      this.Canvas = null;
      this.Width = a;
      this.Height = b;
      options = c || {};
    } else if (isCanvas(a)) {
      this.Canvas = a;
      options = b || {};
    } else if (isCanvas(c)) {
      this.Canvas = c;
      options = d || {};
    } else {
      throw new TypeError('NativeRenderer: expected (width, height), (canvas) or (adapter, device, canvas)');
    }
    if (this.Canvas) {
      this.Width = this.Canvas.width;
      this.Height = this.Canvas.height;
    }
    this.Options = options;
    this.Pipeline = options.pipeline || 'restir';
    if (!(this.Pipeline in PIPELINE)) throw new Error(`unknown pipeline ${this.Pipeline}`);
    this.Handle = null;
    this.PresentSource = 'accum';
    this.createHandle();
    this.World = null;
    this.Skins = new Map(); // mesh -> { first, n, joints, targets } of SetSkin
    this.Camera = null;
    this.FrameCount = 0;
    this.Uniform = null;
    // canvas painting (Render): the 2D context, the present in flight, its waiters
    this.Context2D = undefined;
    this.RenderSerial = 0;
    this.PresentedSerial = 0;
    this.PresentInFlight = null;
    this.PresentWanted = false;
    this.PresentWaiters = [];
    this.PresentError = null;
  }

  /** A handle for this.Width x this.Height (rows rowBegin..rowEnd of it). */
  createHandle() {
    const o = this.Options;
    this.RowBegin = o.rowBegin || 0;
    this.RowEnd = o.rowEnd || this.Height;
    this.Handle = addon.create({
      width: this.Width, height: this.Height, rowBegin: this.RowBegin, rowEnd: this.RowEnd,
      device: o.device === undefined ? -1 : o.device,
      pipeline: PIPELINE[this.Pipeline], flags: o.flags || 0,
      reuseRadius: o.reuseRadius || 0, reuseNeighbors: o.reuseNeighbors || 0,
      temporalCap: o.temporalCap || 0, frameColor: !!o.frameColor,
    });
    // (a new handle has no denoised image yet: the source is applied by its first Denoise)
    this.DenoisedSourceSet = false;
  }

  GetCamera() { return this.Camera; }

  ResetFrameCount() { this.FrameCount = 0; }

  /**
   * Renderer_TEST.Initialize (:141-163): the canvas's current size (a changed size recreates the
   * handle, as DestroyGPUResources + CreateGPUResources do), a new camera at (0,0,6) with
   * yaw / pitch 0, FrameCount 0, the world uploaded.
   */
  async Initialize(world) {
    // a reference World is serialized here (SerializeWorldData); a serialized one is taken as is
    if (world && world.InstancesPool instanceof Map) world = SerializeWorldData(world);
    if (!world || !(world.scene instanceof Uint32Array) || !Array.isArray(world.offsets) || world.offsets.length !== 7) {
      throw new TypeError('Initialize: expected a World or a serialized world {scene, geometry, accel, offsets[7]}');
    }
    if (this.Canvas && (this.Canvas.width !== this.Width || this.Canvas.height !== this.Height)) {
      if (this.Options.rowBegin || this.Options.rowEnd) {
        throw new Error('Initialize: a row-band renderer cannot follow a canvas resize');
      }
      if (!(this.Canvas.width > 0 && this.Canvas.height > 0)) throw new RangeError('Initialize: empty canvas');
      this.dropPresent();
      if (this.Handle) addon.destroy(this.Handle);
      this.Handle = null;
      this.Width = this.Canvas.width;
      this.Height = this.Canvas.height;
      this.createHandle();
    }
    this.Camera = new Camera(this.Width, this.Height);
    this.Camera.SetLocationFromXYZ(0, 0, 6);
    this.Camera.SetYaw(0);
    this.Camera.SetPitch(0);
    this.World = world;
    this.ResetFrameCount();
    addon.uploadScene(this.Handle, world.scene, world.geometry, world.accel);
    this.Skins.clear(); // (the upload drops every skin)
    addon.resetAccumulation(this.Handle);
  }

  /**
   * Edit instances, materials and lights in place (ptx_update_scene): `world` is the world of
   * Initialize with instances moved, turned, scaled or switched to another loaded mesh, materials or
   * lights changed -- the same meshes, counts and offsets, else a RangeError.  Returns the mask of the
   * blocks that changed (1 instances, 2 materials, 4 lights; 0: nothing to do).  Whole-image handles;
   * the frame count is the caller's (ResetFrameCount, as on a camera move).
   */
  UpdateWorld(world) {
    if (world && world.InstancesPool instanceof Map) world = SerializeWorldData(world);
    if (!world || !(world.scene instanceof Uint32Array) || !Array.isArray(world.offsets) || world.offsets.length !== 7) {
      throw new TypeError('UpdateWorld: expected a World or a serialized world {scene, geometry, accel, offsets[7]}');
    }
    if (!this.World) throw new Error('UpdateWorld: Initialize first');
    if (this.Options.rowBegin || this.Options.rowEnd) throw new Error('UpdateWorld: whole-image renderers only');
    const old = this.World;
    const same = world.offsets.every((v, i) => v === old.offsets[i]) && world.instanceCount === old.instanceCount &&
      world.lightCount === old.lightCount && world.scene.length === old.scene.length &&
      world.geometry.length === old.geometry.length && world.accel.length === old.accel.length;
    if (!same) throw new RangeError('UpdateWorld: the edited world has another layout (offsets, counts, geometry or accel length): Initialize uploads it');
    const mask = addon.updateScene(this.Handle, world.scene);
    this.World = world;
    return mask;
  }

  /**
   * Deform a loaded mesh in place (ptx_update_vertices): `records` is a Uint32Array of 8 words per
   * vertex -- position, normal, uv as in the geometry array -- that replace the vertex records
   * [first, first + records.length / 8) of mesh `mesh`.  The library derives the mesh's triangles again
   * and refits its BLAS on the GPU, the topology kept; histories are kept and dropped as by an
   * instance edit.  this.World is afterwards what the handle renders: its geometry rewritten, its
   * accel ReadAccel()'s (new arrays; the world passed to Initialize is not written).  After Update()
   * (the handle needs a frame set); band renderers make the same call on every band; the frame count
   * is the caller's.  A refused call throws and changes nothing.
   */
  UpdateVertices(mesh, first, records) {
    if (!Number.isInteger(mesh) || mesh < 0 || !Number.isInteger(first) || first < 0 || !(records instanceof Uint32Array) ||
        records.length % 8 !== 0) {
      throw new TypeError('UpdateVertices: expected (mesh, first, Uint32Array of 8 words per vertex)');
    }
    if (!this.World) throw new Error('UpdateVertices: Initialize first');
    addon.updateVertices(this.Handle, mesh, first, records);
    if (records.length === 0) return;
    const w = this.World;
    // the mesh's vertex records: word 0 of its descriptor (6 words per mesh at offsets[0]) is their first word
    const geometry = new Uint32Array(w.geometry);
    geometry.set(records, w.scene[w.offsets[0] + 6 * mesh] + 8 * first);
    this.World = Object.assign({}, w, { geometry, accel: this.ReadAccel() });
  }

  /**
   * The accel array as the handle traces it now (ptx_read_accel): the uploaded one with every
   * reachable node's box from the device's tables -- after UpdateVertices, the refit.  Blocking.
   */
  ReadAccel() {
    if (!this.World) throw new Error('ReadAccel: Initialize first');
    const out = new Uint32Array(this.World.accel.length);
    addon.readAccel(this.Handle, out);
    return out;
  }

  /**
   * A mesh's BLAS built on the GPU (ptx_build_blas), in the shapes bvh.js buildBlas produces:
   * {roots: one Uint32Array of 8 words per node per group, indices (and index): the reordered Uint32Array,
   * maxDepth}.  `positions` a Float32Array of 3 per vertex, `indices` a Uint32Array of 3 per triangle, `groups`
   * an array of [firstTriangle, triangleCount]; `options.builder` 'lbvh' (the default) or 'sah' (the host SAH
   * builder's nodes, a leaf's triangles in input order).  Needs no world; changes nothing a frame reads.
   * Blocking; a refused call throws.
   */
  BuildBlas(positions, indices, groups, maxLeafTris = 10, options = {}) {
    const builders = { lbvh: 0, sah: 1 };
    const builder = options && options.builder !== undefined ? options.builder : 'lbvh';
    if (!(positions instanceof Float32Array) || !(indices instanceof Uint32Array) || !Array.isArray(groups) ||
        !Number.isInteger(maxLeafTris) || maxLeafTris < 0 || !Object.prototype.hasOwnProperty.call(builders, builder)) {
      throw new TypeError("BuildBlas: expected (Float32Array, Uint32Array, [[first, count], ...], maxLeafTris, " +
                          "{builder: 'lbvh' | 'sah'})");
    }
    const flat = Uint32Array.from(groups.flat());
    if (flat.length !== 2 * groups.length) throw new TypeError('BuildBlas: a group is [firstTriangle, triangleCount]');
    let worst = 0;
    for (let g = 0; g < groups.length; g++) worst += Math.max(0, 2 * flat[2 * g + 1] - 1);
    const nodes = new Uint32Array(8 * worst);
    const out = new Uint32Array(indices.length);
    const counts = new Uint32Array(groups.length);
    const maxDepth = addon.buildBlas(this.Handle, positions, indices, flat, maxLeafTris, nodes, out, counts, builders[builder]);
    const roots = [];
    let at = 0;
    for (const c of counts) {
      roots.push(nodes.slice(at, at + 8 * c));
      at += 8 * c;
    }
    return { roots, indices: out, index: out, maxDepth };
  }

  /**
   * Build mesh `mesh`'s BLAS again from the vertex records the device holds now and splice it into the handle
   * (ptx_rebuild_mesh): after a pose far from the one the tree was built for, where a refit leaves inflated
   * boxes.  `options.builder` 'sah' (the default) or 'lbvh', `options.maxLeafTris` (10).  Skins, the
   * accumulation and the denoiser's history stay; the reuse history is dropped.  Returns {nAccel, meshNodes,
   * maxDepth, sceneWords}; this.World is afterwards what the handle renders -- its scene, geometry and accel
   * replaced by new arrays (ptx_read_scene; the accel array's length and later meshes' descriptors may have
   * moved).  After Update(); band renderers make the same call on every band.  A refused call throws and
   * changes nothing.
   */
  RebuildMesh(mesh, options = {}) {
    const builders = { lbvh: 0, sah: 1 };
    const builder = options && options.builder !== undefined ? options.builder : 'sah';
    const maxLeafTris = options && options.maxLeafTris !== undefined ? options.maxLeafTris : 10;
    if (!Number.isInteger(mesh) || mesh < 0 || !Number.isInteger(maxLeafTris) || maxLeafTris < 0 ||
        !Object.prototype.hasOwnProperty.call(builders, builder)) {
      throw new TypeError("RebuildMesh: expected (mesh, {builder: 'sah' | 'lbvh', maxLeafTris})");
    }
    if (!this.World) throw new Error('RebuildMesh: Initialize first');
    const info = addon.rebuildMesh(this.Handle, mesh, builders[builder], maxLeafTris);
    const { scene, geometry, accel } = addon.readScene(this.Handle);
    this.World = Object.assign({}, this.World, { scene, geometry, accel });
    return info;
  }

  /**
   * The surface-area cost of mesh `mesh`'s trees as the device holds them now (ptx_blas_cost; traversal 1,
   * triangle 1.25, each node's area relative to its root's): it grows as refits inflate the boxes and tells
   * when RebuildMesh pays.  Blocking; changes nothing.
   */
  BlasCost(mesh) {
    if (!Number.isInteger(mesh) || mesh < 0) throw new TypeError('BlasCost: expected a mesh index');
    if (!this.World) throw new Error('BlasCost: Initialize first');
    return addon.blasCost(this.Handle, mesh);
  }

  /**
   * Bind a skin to the vertices [first, first + joints.length / 4) of mesh `mesh` (ptx_set_skin): `joints`
   * a Uint32Array and `weights` a Float32Array of four per vertex; optional Float32Arrays `bind` (six per
   * vertex: position, normal; null: the records as the handle holds them now), `targets` (morph position
   * deltas, 3 per vertex, target after target) and `targetNormals` (the same shape).  The joint count is
   * 1 + the largest index.  Empty arrays remove the mesh's skin.  Nothing a frame reads changes; a
   * refused call throws and binds nothing.  After Update() (the handle needs a frame set).
   */
  SetSkin(mesh, first, joints, weights, bind = null, targets = null, targetNormals = null) {
    const f32 = (a) => a === null || a === undefined || a instanceof Float32Array;
    if (!Number.isInteger(mesh) || mesh < 0 || !Number.isInteger(first) || first < 0 || !(joints instanceof Uint32Array) ||
        joints.length % 4 !== 0 || !(weights instanceof Float32Array) || weights.length !== joints.length ||
        !f32(bind) || !f32(targets) || !f32(targetNormals)) {
      throw new TypeError('SetSkin: expected (mesh, first, Uint32Array and Float32Array of 4 per vertex, Float32Arrays or null)');
    }
    const n = joints.length / 4;
    if ((bind && bind.length !== 6 * n) || (targets && (n === 0 || targets.length === 0 || targets.length % (3 * n) !== 0)) ||
        (targetNormals && (!targets || targetNormals.length !== targets.length))) {
      throw new TypeError('SetSkin: bind has 6 floats per vertex, targets 3 per vertex and target, targetNormals the shape of targets');
    }
    if (!this.World) throw new Error('SetSkin: Initialize first');
    let nJoints = 1;
    for (let i = 0; i < joints.length; i++) nJoints = Math.max(nJoints, joints[i] + 1);
    addon.setSkin(this.Handle, mesh, first, nJoints, joints, weights, bind || null, targets || null, targetNormals || null);
    if (n) this.Skins.set(mesh, { first, n, joints: nJoints, targets: targets ? targets.length / (3 * n) : 0 });
    else this.Skins.delete(mesh);
  }

  /**
   * Pose the skinned range of mesh `mesh` and refit its BLAS on the GPU (ptx_skin_vertices): `palette` is
   * a Float32Array of 12 per joint (three rows of four, row-major), `targetWeights` a Float32Array of one
   * per bound morph target (null without targets).  this.World is afterwards what the handle renders:
   * the range's records ReadVertices()'s, the accel array ReadAccel()'s (new arrays).  Blocking; band
   * renderers make the same call on every band.  A refused call throws and changes nothing.
   */
  SkinVertices(mesh, palette, targetWeights = null) {
    if (!Number.isInteger(mesh) || mesh < 0 || !(palette instanceof Float32Array) || palette.length % 12 !== 0 ||
        !(targetWeights === null || targetWeights === undefined || targetWeights instanceof Float32Array)) {
      throw new TypeError('SkinVertices: expected (mesh, Float32Array of 12 per joint, Float32Array of target weights or null)');
    }
    const skin = this.Skins.get(mesh);
    if (!skin) throw new Error(`SkinVertices: mesh ${mesh} has no skin`);
    if (palette.length < 12 * skin.joints || (targetWeights ? targetWeights.length : 0) !== skin.targets) {
      throw new RangeError(`SkinVertices: the skin has ${skin.joints} joints and ${skin.targets} morph targets`);
    }
    addon.skinVertices(this.Handle, mesh, palette.subarray(0, 12 * skin.joints), targetWeights || null);
    const w = this.World;
    const geometry = new Uint32Array(w.geometry);
    geometry.set(this.ReadVertices(mesh, skin.first, skin.n), w.scene[w.offsets[0] + 6 * mesh] + 8 * skin.first);
    this.World = Object.assign({}, w, { geometry, accel: this.ReadAccel() });
  }

  /** The device's current records [first, first + n) of mesh `mesh`, 8 words each (ptx_read_vertices).  Blocking. */
  ReadVertices(mesh, first, n) {
    if (!Number.isInteger(mesh) || mesh < 0 || !Number.isInteger(first) || first < 0 || !Number.isInteger(n) || n < 0) {
      throw new TypeError('ReadVertices: expected (mesh, first, n)');
    }
    if (!this.World) throw new Error('ReadVertices: Initialize first');
    const out = new Uint32Array(8 * n);
    addon.readVertices(this.Handle, mesh, first, out);
    return out;
  }

  /** Renderer_TEST.Update (:165-206): FrameCount++, then the uniform block. */
  Update() {
    this.FrameCount++;
    this.Uniform = buildUniform(this.Width, this.Height, this.Camera, this.FrameCount, this.World);
    addon.setFrame(this.Handle, this.Uniform);
  }

  /**
   * Renderer_TEST.Render (:208-261): all passes + accumulation, asynchronous on the GPU, then the
   * render pass into the canvas (:233-258) when it has a 2D context -- enqueued behind the frame,
   * painted when its bytes land (the event loop is never blocked).
   */
  Render() {
    addon.render(this.Handle);
    this.RenderSerial++;
    if (this.PresentSource === 'accum') this.paint();  // ('denoised': the Denoise() after this frame paints)
  }

  paint() {
    if (this.context2D()) {
      if (this.PresentInFlight) this.PresentWanted = true;
      else this.startPresent();
    }
  }

  /**
   * ptx_denoise behind the frame last rendered (include/ptx.h): {iterations, sigmaLum, sigmaPlane,
   * temporal, alphaMin, followVertices}, every field optional (0 = the default).  temporal: the frame
   * colours integrated over the calls, their history reprojected across camera moves (a renderer made
   * with {frameColor: true}); a ResetFrameCount() keeps that history.  followVertices (with temporal): a
   * pixel on a mesh that UpdateVertices / SkinVertices deformed since the previous temporal call looks its
   * history up where that surface point was then.  With the source 'denoised' the canvas is painted from
   * the result.
   */
  Denoise(opts) {
    addon.denoise(this.Handle, opts || {});
    this.paintDenoised();
  }

  /**
   * ptx_upsample (include/ptx.h): the denoised image of `lo` -- a NativeRenderer of 1/2, 1/3 or 1/4
   * this one's size with the same scene and camera, after its Denoise() -- written at this
   * renderer's size under this renderer's G-buffer as it stands (a RunPass of the G-buffer pass or
   * a frame first); {sigmaPlane} optional.  With the source 'denoised' the canvas is painted from
   * the result, as after Denoise().
   */
  Upsample(lo, opts) {
    addon.upsample(this.Handle, lo.Handle, opts || {});
    this.paintDenoised();
  }

  /**
   * ptx_upsample_temporal (include/ptx.h): Upsample for a `lo` whose frame was rendered through phase
   * (px, py) of every s x s block of this renderer's pixels -- lo.SetPhaseOf(this, s, px, py) instead of
   * its Update() -- integrated over the calls: each small pixel's value goes where it was sampled, the
   * rest is interpolated, the history follows camera moves.  {px, py, sigmaPlane, alphaMin, alphaFill},
   * every field optional.  With the source 'denoised' the canvas is painted from the result.
   */
  UpsampleTemporal(lo, opts) {
    addon.upsampleTemporal(this.Handle, lo.Handle, opts || {});
    this.paintDenoised();
  }

  /**
   * ptx_upsample_follow: this full-size renderer's UpsampleTemporal follows moved instances and deformed or
   * skinned meshes.  From the first UpsampleTemporal made with it on, UpdateWorld, UpdateVertices and
   * SkinVertices keep the history and the next call looks a moved surface's history up where it was; off (the
   * default) an instance edit and a vertex update drop it.  No GPU work.
   */
  SetUpsampleFollow(on) {
    addon.upsampleFollow(this.Handle, !!on);
    this.UpsampleFollow = !!on;
  }

  /**
   * ptx_phase_uniform: this (small) renderer's frame looks through pixel (px, py) of every s x s block
   * of `hi`'s current frame (its Uniform, frame index included); call it where Update() would be.
   */
  SetPhaseOf(hi, s, px, py) {
    this.Uniform = addon.phaseUniform(hi.Uniform, s, px, py);
    addon.setFrame(this.Handle, this.Uniform);
  }

  /** {H.rgb, n} of the last UpsampleTemporal(): the integrated colour and own-sample count, RGBA f32. */
  ReadUpsampleHistory(out) {
    const img = out || new Float32Array((this.RowEnd - this.RowBegin) * this.Width * 4);
    addon.readBuffer(this.Handle, BUF.UPSAMPLE_HISTORY, img);
    return img;
  }

  paintDenoised() {
    if (this.PresentSource !== 'denoised') return;
    if (!this.DenoisedSourceSet) {
      addon.presentSource(this.Handle, BUF.DENOISED);
      this.DenoisedSourceSet = true;
    }
    this.paint();
  }

  /** What Render()'s paint and Present() show: 'accum' (the default) or 'denoised' (see Denoise). */
  SetPresentSource(source) {
    if (source !== 'accum' && source !== 'denoised') throw new Error(`unknown present source ${source}`);
    if (source === 'accum' && this.PresentSource !== 'accum') {
      addon.presentSource(this.Handle, BUF.ACCUM);
      this.DenoisedSourceSet = false;
    }
    this.PresentSource = source;
  }

  /** The denoised image of the last Denoise(), RGBA f32. */
  ReadDenoised(out) {
    const img = out || new Float32Array((this.RowEnd - this.RowBegin) * this.Width * 4);
    addon.readBuffer(this.Handle, BUF.DENOISED, img);
    return img;
  }

  /** The canvas's 2D context (looked up once; null when the canvas has none, e.g. in a worker). */
  context2D() {
    if (this.Context2D === undefined) {
      const c = this.Canvas;
      this.Context2D = (c && typeof c.getContext === 'function' && c.getContext('2d')) || null;
    }
    return this.Context2D;
  }

  startPresent() {
    const ctx = this.context2D();
    const w = this.Canvas.width, h = this.Canvas.height;
    this.PresentWanted = false;
    if (!(w > 0 && h > 0)) return;  // (nothing to paint on an empty canvas)
    let image;
    try {
      image = ctx.createImageData(w, h);
      addon.presentAsync(this.Handle, w, h, false);
    } catch (e) {  // painting never breaks the render loop: the error is kept for the host to read
      this.PresentError = e;
      return;
    }
    this.PresentInFlight = { serial: this.RenderSerial, image, handle: this.Handle };
    soon(() => this.pollPresent(0));
  }

  pollPresent(tries) {
    const f = this.PresentInFlight;
    if (!f || f.handle !== this.Handle) return;  // dropped (Destroy, a resize)
    let done;
    try {
      done = addon.presentPoll(this.Handle, f.image.data);
    } catch (e) {
      if (/in flight on this handle/.test(String(e && e.message))) {  // a RenderAsync owns the handle
        setTimeout(() => this.pollPresent(tries + 1), 1);
        return;
      }
      this.PresentInFlight = null;
      this.PresentError = e;
      this.settlePresent();
      return;
    }
    if (!done) {  // the first few polls on the next turns, then every millisecond
      if (tries < 8) soon(() => this.pollPresent(tries + 1));
      else setTimeout(() => this.pollPresent(tries + 1), 1);
      return;
    }
    this.PresentInFlight = null;
    this.PresentedSerial = f.serial;
    this.context2D().putImageData(f.image, 0, 0);
    if (this.PresentWanted) this.startPresent();
    else this.settlePresent();
  }

  settlePresent() {
    const ws = this.PresentWaiters;
    this.PresentWaiters = [];
    for (const r of ws) r();
  }

  /** Resolves once no present is in flight (the canvas shows the newest rendered frame). */
  PresentIdle() {
    if (!this.PresentInFlight) return Promise.resolve(this.PresentedSerial);
    return new Promise((resolve) => this.PresentWaiters.push(() => resolve(this.PresentedSerial)));
  }

  dropPresent() {
    this.PresentInFlight = null;
    this.PresentWanted = false;
    this.settlePresent();
  }

  /** Render off the event loop; resolves once the frame (and the optional copy) is done. */
  RenderAsync(out) { return addon.renderAsync(this.Handle, out || null); }

  /** The accumulated band image, RGBA f32 (the reference's Scene texture). */
  ReadImage(out) {
    const img = out || new Float32Array((this.RowEnd - this.RowBegin) * this.Width * 4);
    addon.readBuffer(this.Handle, BUF.ACCUM, img);
    return img;
  }

  /**
   * Renderer_TEST.Render's render pass (Renderer_TEST.ts:233-255) onto a canvasW x canvasH canvas
   * (default: the image size): Uint8ClampedArray of canvasW * canvasH * 4 bytes, RGBA (bgra false:
   * ImageData for putImageData) or BGRA (bgra true); row 0 = the canvas's top row.
   */
  Present(canvasW = this.Width, canvasH = this.Height, bgra = false, out = null) {
    const px = out || new Uint8ClampedArray(canvasW * canvasH * 4);
    addon.present(this.Handle, canvasW, canvasH, bgra, px);
    return px;
  }

  RunPass(pass) { addon.runPass(this.Handle, pass); }
  Synchronize() { addon.synchronize(this.Handle); }
  GetStats() { return addon.getStats(this.Handle); }
  Trace(rays, hits, epsMode = 1) { addon.trace(this.Handle, rays, hits, epsMode); }

  /** DestroyGPUResources (:462-476). */
  Destroy() {
    this.dropPresent();
    if (this.Handle) addon.destroy(this.Handle);
    this.Handle = null;
  }
}

/**
 * The same render pass on the host, for a frame gathered from row bands (Renderer.renderBands'
 * image, rows 0 .. height): canvas pixel (x, y) shows texel (floor((2x+1)*600 / 2canvasW),
 * floor((2canvasH-2y-1)*450 / 2canvasH)) -- FragmentShader.wgsl:7-10's PixelUV * (600, 450) of the
 * quad's VertexShader.wgsl UV at the pixel centre, in exact integers -- clamped to [0, 1] and
 * rounded half to even to unorm8 (ptx_present's rules; out-of-bounds texels read 0).
 */
function presentImage(img, width, height, canvasW, canvasH, bgra = false, out = null) {
  const px = out || new Uint8ClampedArray(canvasW * canvasH * 4);
  const f = new Float32Array(1);
  const unorm8 = (x) => {
    if (!(x > 0)) return 0; // (NaN, <= 0)
    if (x >= 1) return 255;
    f[0] = Math.fround(x * 255); // the f32 product, then round half to even
    const v = f[0], fl = Math.floor(v), d = v - fl;
    return d > 0.5 || (d === 0.5 && (fl % 2) === 1) ? fl + 1 : fl;
  };
  for (let y = 0; y < canvasH; y++) {
    const ty = Math.floor(((2 * canvasH - 2 * y - 1) * 450) / (2 * canvasH));
    for (let x = 0; x < canvasW; x++) {
      const tx = Math.floor(((2 * x + 1) * 600) / (2 * canvasW));
      const o = 4 * (y * canvasW + x);
      let r = 0, g = 0, b = 0;
      if (tx < width && ty < height) {
        const i = 4 * (ty * width + tx);
        r = unorm8(img[i]); g = unorm8(img[i + 1]); b = unorm8(img[i + 2]);
      }
      px[o] = bgra ? b : r; px[o + 1] = g; px[o + 2] = bgra ? r : b; px[o + 3] = 255;
    }
  }
  return px;
}

module.exports = { NativeRenderer, buildUniform, presentImage, addon, PASS, BUF, FLAGS, UNIFORM_WORDS };
