'use strict';
// Deforming a mesh in place through the drop-in (INTEGRATION.md, "Deforming a mesh"): a NativeRenderer
// renders a frame of a serialised world, takes new vertex records for one mesh through
// UpdateVertices(mesh, first, records), reads the refitted accel array back and renders the next frame.
//
// argv: JSON {sceneDir, records: file of u32 vertex records, mesh, first, width, height, pipeline, out}
// stdout: JSON {before: ReadAccel() equals the uploaded array, worldAccel: this.World.accel equals ReadAccel(),
//               geometryChanged: words of this.World.geometry that differ from the uploaded array,
//               untouched: the world passed to Initialize kept its arrays, refused: [messages],
//               uniform: [33 words of the last frame], keys: [...Object.keys(addon)]};
// ReadAccel() after the update goes to `${out}.accel.u32`, this.World.geometry to `${out}.geometry.u32`,
// ReadImage() of the frame after it to `${out}.f32`.
const fs = require('fs');
const { NativeRenderer, addon } = require('../../pathtracerdemo_amd/js/NativeRenderer');
const { loadCompiledScene } = require('../../pathtracerdemo_amd/js/scene_io');

const same = (a, b) => a.length === b.length && a.every((v, i) => v === b[i]);

async function main() {
  const req = JSON.parse(process.argv[2]);
  const world = loadCompiledScene(req.sceneDir);
  const uploaded = { geometry: Uint32Array.from(world.geometry), accel: Uint32Array.from(world.accel) };
  const bytes = fs.readFileSync(req.records);
  const records = new Uint32Array(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength));
  const r = new NativeRenderer(req.width, req.height, { pipeline: req.pipeline, device: 0 });
  await r.Initialize(world);
  r.Update();
  r.Render();
  const before = same(r.ReadAccel(), uploaded.accel);
  const refused = [];
  const nan = Uint32Array.from(records.subarray(0, 16));
  nan[9] = 0x7fc00000;
  for (const call of [() => r.UpdateVertices(req.mesh, req.first + 1, records), () => r.UpdateVertices(99, 0, records.subarray(0, 8)),
    () => r.UpdateVertices(req.mesh, 0, nan), () => r.UpdateVertices(req.mesh, 0, records.subarray(0, 7)),
    () => r.UpdateVertices(req.mesh, 0, new Float32Array(8))]) {
    try { call(); refused.push(null); } catch (e) { refused.push(`${e.name}: ${e.message}`); }
  }
  const stillUploaded = same(r.ReadAccel(), uploaded.accel) && r.World === world;
  r.UpdateVertices(req.mesh, req.first, records);
  const accel = r.ReadAccel();
  let geometryChanged = 0;
  for (let i = 0; i < uploaded.geometry.length; i++) geometryChanged += r.World.geometry[i] !== uploaded.geometry[i] ? 1 : 0;
  const res = {
    before, stillUploaded, worldAccel: same(r.World.accel, accel), geometryChanged,
    untouched: same(world.geometry, uploaded.geometry) && same(world.accel, uploaded.accel), refused,
  };
  fs.writeFileSync(`${req.out}.accel.u32`, Buffer.from(accel.buffer));
  fs.writeFileSync(`${req.out}.geometry.u32`, Buffer.from(r.World.geometry.buffer));
  r.Update();
  r.Render();
  fs.writeFileSync(`${req.out}.f32`, Buffer.from(r.ReadImage().buffer));
  res.uniform = Array.from(r.Uniform);
  res.keys = Object.keys(addon);
  r.Destroy();
  process.stdout.write(JSON.stringify(res));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
