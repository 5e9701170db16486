'use strict';
// Rebuilding a loaded mesh through the drop-in (INTEGRATION.md, "Rebuilding a mesh"): a NativeRenderer renders a
// frame of a serialised world, binds a skin, poses it far from the bind pose, asks BlasCost what the refit left,
// rebuilds the mesh's BLAS with RebuildMesh and renders the next frame.
//
// argv: JSON {sceneDir, dir: directory with joints.u32, weights.f32, bind.f32, palette.f32, mesh, builder, width,
//             height, pipeline, out}
// stdout: JSON {costs: [at upload, after the pose, after the rebuild], info: RebuildMesh's, newArrays: this.World's
//               three arrays are new objects, untouched: the world passed to Initialize kept its arrays, refused:
//               [messages], uniform: [33 words of the last frame], keys: [...Object.keys(addon)]};
// this.World's arrays after the rebuild go to `${out}.scene.u32`, `${out}.geometry.u32` and `${out}.accel.u32`,
// ReadImage() of the frame after it to `${out}.f32`.
const fs = require('fs');
const path = require('path');
const { NativeRenderer, addon } = require('../../pathtracerdemo_amd/js/NativeRenderer');
const { loadCompiledScene } = require('../../pathtracerdemo_amd/js/scene_io');

const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);
function load(file, Type) {
  const bytes = fs.readFileSync(file);
  return new Type(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength));
}

async function main() {
  const req = JSON.parse(process.argv[2]);
  const world = loadCompiledScene(req.sceneDir);
  const uploaded = { scene: Uint32Array.from(world.scene), geometry: Uint32Array.from(world.geometry), accel: Uint32Array.from(world.accel) };
  const f = (name, Type) => load(path.join(req.dir, name), Type);
  const joints = f('joints.u32', Uint32Array), weights = f('weights.f32', Float32Array), bind = f('bind.f32', Float32Array);
  const palette = f('palette.f32', Float32Array);
  const r = new NativeRenderer(req.width, req.height, { pipeline: req.pipeline, device: 0 });
  await r.Initialize(world);
  r.Update();
  r.Render();
  const costs = [r.BlasCost(req.mesh)];
  r.SetSkin(req.mesh, 0, joints, weights, bind);
  r.SkinVertices(req.mesh, palette, null);
  costs.push(r.BlasCost(req.mesh));
  const refused = [];
  const attempt = (call) => { try { call(); refused.push(null); } catch (e) { refused.push(`${e.name}: ${e.message}`); } };
  const posed = r.World;
  attempt(() => r.RebuildMesh(99));                                   // a mesh that is not loaded
  attempt(() => addon.rebuildMesh(r.Handle, req.mesh, 2, 0));         // a builder the library does not know
  attempt(() => addon.rebuildMesh(r.Handle, req.mesh, 1, 65));        // max_leaf above 64
  attempt(() => r.RebuildMesh(req.mesh, { builder: 'median' }));      // the drop-in's own argument errors
  attempt(() => r.RebuildMesh(1.5));
  attempt(() => r.BlasCost(99));
  attempt(() => addon.blasCost(r.Handle));
  const stillPosed = r.World === posed;
  const info = r.RebuildMesh(req.mesh, { builder: req.builder });
  costs.push(r.BlasCost(req.mesh));
  const w = r.World;
  const res = {
    costs, info, refused, stillPosed,
    newArrays: w.scene !== posed.scene && w.geometry !== posed.geometry && w.accel !== posed.accel,
    readAccel: same(r.ReadAccel(), w.accel),
    untouched: same(world.scene, uploaded.scene) && same(world.geometry, uploaded.geometry) && same(world.accel, uploaded.accel),
  };
  for (const name of ['scene', 'geometry', 'accel']) fs.writeFileSync(`${req.out}.${name}.u32`, Buffer.from(w[name].buffer));
  r.Update();
  r.Render();
  fs.writeFileSync(`${req.out}.f32`, Buffer.from(r.ReadImage().buffer));
  res.uniform = Array.from(r.Uniform);
  res.keys = Object.keys(addon);
  r.Destroy();
  process.stdout.write(JSON.stringify(res));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
